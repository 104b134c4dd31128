// url_full_check.cpp — the in-place url.Parse (odigos_amd/csrc/url_full.hpp,
// its host instantiation) against go_url_parse_path (urlparse.cpp), a plain
// host program built with -fsanitize=address,undefined by
// tests/test_url_full_host.py.  argv[1]: a file of hex-encoded strings, one
// per line (the hand-written list and the reference's KAT strings).  Then
// every string of length 0-4 over "a/:?#%@[]2 ." and 100,000 seeded strings
// from a URL grammar with 0-2 random byte substitutions or insertions.  For
// every string: the outcome class, the sub-range and the decoded bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../odigos_amd/csrc/url_full.hpp"
#include "../odigos_amd/csrc/urlparse.hpp"

using namespace ose;

namespace {
long g_checked = 0, g_failed = 0;

std::string show(const std::string& s) {
  std::string o;
  char buf[8];
  for (unsigned char c : s) {
    if (c >= 0x20 && c < 0x7F && c != '\\') o += (char)c;
    else { snprintf(buf, sizeof buf, "\\x%02x", c); o += buf; }
  }
  return o;
}

// the outcome class from go_url_parse_path alone: the Path is a suffix of the
// URL before its '#' and '?' unless it was unescaped
uint32_t ref_class(const std::string& raw, bool ok, const std::string& path) {
  if (!ok) return urlfull::kError;
  if (path.empty()) return urlfull::kEmpty;
  std::string cut = raw.substr(0, raw.find('#'));
  cut = cut.substr(0, cut.find('?'));
  if (cut.size() >= path.size() && cut.compare(cut.size() - path.size(), path.size(), path) == 0) return urlfull::kInPlace;
  return urlfull::kDecoded;
}

// one string; returns the reference's class
uint32_t check(const std::string& raw) {
  std::string want;
  const bool ok = go_url_parse_path(raw, want);
  const uint32_t cls = ref_class(raw, ok, want);
  // the parser reads [off, off + len) of a larger buffer: no byte outside it
  // (the exact-size copy puts ASan's redzones at both ends)
  const uint32_t pad = 3;
  std::vector<char> buf(raw.size() + 2 * pad, '%');
  std::vector<char> exact(raw.begin(), raw.end());
  urlfull::ViewSrc src{exact.data()};
  const urlfull::Result r = urlfull::parse(src, 0, (uint32_t)raw.size());
  for (size_t k = 0; k < raw.size(); k++) buf[pad + k] = raw[k];
  urlfull::ViewSrc src2{buf.data()};
  const urlfull::Result r2 = urlfull::parse(src2, pad, (uint32_t)raw.size());
  g_checked++;
  std::string why;
  if (r2.outcome != r.outcome || r2.len != r.len || r2.dec_len != r.dec_len ||
      (r.outcome >= urlfull::kInPlace && r2.off != r.off + pad))
    why = "the result depends on the offset";
  else if (r.outcome != cls) why = "outcome class";
  else if (r.outcome != urlfull::kError && (uint64_t)r.off + r.len > raw.size()) why = "sub-range out of bounds";
  else if (r.outcome == urlfull::kInPlace && (r.len == 0 || raw.compare(r.off, r.len, want) != 0 || r.len != want.size()))
    why = "in-place sub-range";
  else if (r.outcome == urlfull::kEmpty && r.len != 0) why = "empty with a length";
  else if (r.outcome == urlfull::kDecoded) {
    if (r.dec_len != want.size() || raw.substr(r.off, r.len).find('%') == std::string::npos) {
      why = "decoded length";
    } else {
      std::vector<uint8_t> out(r.dec_len);   // exactly dec_len bytes: a longer write is an ASan error
      urlfull::unescape_into(src, r.off, r.len, out.data());
      if (std::string(out.begin(), out.end()) != want) why = "decoded bytes";
    }
  }
  if (!why.empty() && g_failed++ < 20)
    printf("MISMATCH (%s): \"%s\": reference ok=%d path=\"%s\", parser outcome=%u [%u,+%u) dec_len=%u\n", why.c_str(),
           show(raw).c_str(), (int)ok, show(want).c_str(), r.outcome, r.off, r.len, r.dec_len);
  return cls;
}

struct Rng {   // splitmix64: the corpus is the same on every platform
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
  bool pct(uint32_t p) { return below(100) < p; }
  template <size_t N>
  const char* pick(const char* const (&a)[N]) { return a[below((uint32_t)N)]; }
};

std::string word(Rng& g, uint32_t valid_escape, uint32_t bad_escape) {
  static const char* const kWords[] = {"user", "1234", "api", "v1", "a", "index.html", "x-y_z~", "caf\xc3\xa9", "a:b", "a@b", ""};
  static const char* const kEsc[] = {"%20", "%2F", "%2f", "%41", "%e2%82%ac", "%25", "%00", "%7e"};
  static const char* const kBad[] = {"%", "%4", "%zz", "%4g", "%g4"};
  std::string w = g.pick(kWords);
  if (g.pct(valid_escape)) w.insert(g.below((uint32_t)w.size() + 1), g.pick(kEsc));
  if (g.pct(bad_escape)) w.insert(g.below((uint32_t)w.size() + 1), g.pick(kBad));
  return w;
}

std::string grammar(Rng& g) {
  static const char* const kSchemes[] = {"http", "https", "HTTP", "a+b-c.d", "x", "ws"};
  static const char* const kHosts[] = {"example.com", "h", "10.0.0.1", "[::1]", "[fe80::1%25en0]", "[fe80::1%25e%20n]",
                                        "h%25", "caf\xc3\xa9.fr", "h%c3%a9", "", "a_b", "h%41", "[::1", "h x", "[fe80::1%25e%2fn]"};
  static const char* const kPorts[] = {":80", ":8080", ":", ":80a", ":x"};
  static const char* const kUsers[] = {"u", "u:p", "u%41:p", "u:p%4", "u^", "a@b", "u:", ""};
  std::string s;
  const bool scheme = g.pct(55);
  if (scheme) { s += g.pick(kSchemes); s += ':'; }
  const bool authority = g.pct(scheme ? 80 : 30);
  if (authority) {
    s += "//";
    if (g.pct(15)) { s += g.pick(kUsers); s += '@'; }
    s += g.pick(kHosts);
    if (g.pct(25)) s += g.pick(kPorts);
  }
  // segments: absolute after an authority; else absolute, relative or (with a scheme) opaque
  const uint32_t nseg = g.below(4);
  const bool leading = authority || g.pct(75);
  for (uint32_t k = 0; k < nseg; k++) {
    if (k || leading) s += '/';
    s += word(g, 18, 2);
  }
  if (g.pct(30)) { s += '?'; s += word(g, 30, 10); if (g.pct(30)) { s += "=?"; s += word(g, 0, 0); } }
  if (g.pct(20)) { s += '#'; s += word(g, 30, 6); }
  // 0-2 random byte substitutions or insertions
  static const char kBytes[] = "a/:?#%@[]2 .*\x7f\x1f\x80\xff";
  for (uint32_t m = g.below(8) < 5 ? 0 : 1 + g.below(2); m > 0; m--) {
    const char c = g.pct(80) ? kBytes[g.below(sizeof kBytes - 1)] : (char)g.below(256);
    if (!s.empty() && g.pct(50)) s[g.below((uint32_t)s.size())] = c;
    else s.insert(s.begin() + g.below((uint32_t)s.size() + 1), c);
  }
  return s;
}

int unhex1(char c) { return c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10; }
}  // namespace

int main(int argc, char** argv) {
  // 1. the listed strings
  long listed = 0;
  if (argc > 1) {
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
      std::string s;
      for (size_t k = 0; k + 1 < line.size(); k += 2) s += (char)(unhex1(line[k]) << 4 | unhex1(line[k + 1]));
      check(s);
      listed++;
    }
  }
  // 2. every string of length 0-4 over the alphabet
  const std::string alpha = "a/:?#%@[]2 .";
  long exhaustive = 0;
  for (uint32_t len = 0; len <= 4; len++) {
    uint64_t count = 1;
    for (uint32_t k = 0; k < len; k++) count *= alpha.size();
    for (uint64_t v = 0; v < count; v++) {
      std::string s(len, ' ');
      uint64_t x = v;
      for (uint32_t k = 0; k < len; k++) { s[k] = alpha[x % alpha.size()]; x /= alpha.size(); }
      check(s);
      exhaustive++;
    }
  }
  // 3. the grammar corpus; every outcome at least 5% of it
  Rng g{20260213};
  const long kCorpus = 100000;
  long cls[4] = {0, 0, 0, 0};
  for (long k = 0; k < kCorpus; k++) cls[check(grammar(g))]++;
  printf("listed %ld, exhaustive %ld, grammar %ld: error %.1f%% empty %.1f%% in-place %.1f%% decoded %.1f%%\n", listed,
         exhaustive, kCorpus, 100.0 * cls[0] / kCorpus, 100.0 * cls[1] / kCorpus, 100.0 * cls[2] / kCorpus,
         100.0 * cls[3] / kCorpus);
  bool ok = g_failed == 0 && exhaustive == 22621;
  for (int c = 0; c < 4; c++)
    if (cls[c] * 20 < kCorpus) { printf("outcome %d is under 5%% of the grammar corpus\n", c); ok = false; }
  printf("%ld strings, %ld mismatches\n", g_checked, g_failed);
  if (!ok) return 1;
  printf("OK\n");
  return 0;
}
