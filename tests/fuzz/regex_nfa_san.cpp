// regex_nfa_san.cpp — stand-alone ASan + UBSan driver of the NFA route
// (regex_nfa.hpp): compile_nfa, nfa_image and regex_nfa_device.hpp's match()
// as the kernels and osehost_regex_nfa_match compile them.  Built and run by
// tests/fuzz/run_regex_nfa_san.py with the product's regex sources; no Python
// and no device in the process.
//
// Input file: cases of { u32 pattern_len, pattern, u32 n, n x { u32 len,
// bytes, u8 expected } }.  Every string is copied into an allocation of
// exactly its length, so a read past its end is reported.  After the given
// strings each pattern runs over seeded random byte strings (invalid UTF-8,
// a multibyte rune truncated at the end) and is compared with the DFA where
// one compiles within small caps.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../odigos_amd/csrc/regex_dfa.hpp"
#include "../../odigos_amd/csrc/regex_nfa.hpp"

namespace {

struct In {
  std::vector<uint8_t> b;
  size_t p = 0;
  bool u32(uint32_t& v) {
    if (p + 4 > b.size()) return false;
    std::memcpy(&v, b.data() + p, 4);
    p += 4;
    return true;
  }
  bool bytes(uint32_t n, std::vector<uint8_t>& out) {
    if (p + n > b.size()) return false;
    out.assign(b.begin() + p, b.begin() + p + n);
    p += n;
    return true;
  }
};

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}

bool run(const std::vector<uint8_t>& image, const std::vector<uint8_t>& s) {
  // exact-size heap copy: the matcher may read [0, n) only
  uint8_t* q = new uint8_t[s.size() ? s.size() : 1];
  if (!s.empty()) std::memcpy(q, s.data(), s.size());
  const bool r = ose::nfa_match(image, q, s.size());
  delete[] q;
  return r;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  In in;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) in.b.insert(in.b.end(), buf, buf + n);
    std::fclose(f);
  }
  static const char* kTails[] = {"\xc3", "\xe4\xb8", "\xe4", "\xf0\x9f\x98", "\xff", "\xed\xa0\x80", "\xe4\xb8\x80"};
  uint64_t patterns = 0, strings = 0, mismatches = 0;
  uint32_t plen;
  while (in.u32(plen)) {
    std::vector<uint8_t> pb;
    uint32_t n;
    if (!in.bytes(plen, pb) || !in.u32(n)) return 2;
    const std::string pattern(pb.begin(), pb.end());
    ose::NfaProgram prog;
    std::string err;
    const ose::RegexStatus st = ose::compile_nfa(pattern, prog, err);
    if (st != ose::RegexStatus::Ok) {
      std::printf("compile_nfa refused `%s`: %s\n", pattern.c_str(), err.c_str());
      return 1;
    }
    const std::vector<uint8_t> image = ose::nfa_image(prog);
    patterns++;
    for (uint32_t k = 0; k < n; k++) {
      uint32_t len;
      std::vector<uint8_t> s;
      if (!in.u32(len) || !in.bytes(len, s) || in.p >= in.b.size()) return 2;
      const bool want = in.b[in.p++] != 0;
      strings++;
      if (run(image, s) != want) {
        mismatches++;
        std::printf("mismatch `%s` on %u bytes\n", pattern.c_str(), len);
      }
    }
    ose::Dfa dfa;
    std::string derr;
    const bool have_dfa = ose::compile_dfa(pattern, dfa, derr, 4096, 1 << 20) == ose::RegexStatus::Ok;
    for (int k = 0; k < 64; k++) {
      std::vector<uint8_t> s;
      const uint32_t len = rnd() % 48;
      for (uint32_t q = 0; q < len; q++) {
        const uint32_t r = rnd();
        s.push_back((r & 7) == 0 ? (uint8_t)(r >> 8) : (uint8_t)("ab\n_ c9"[(r >> 8) % 7]));
      }
      if (k & 1) {
        const char* t = kTails[(k >> 1) % 7];
        s.insert(s.end(), t, t + std::strlen(t));
      }
      strings++;
      const bool got = run(image, s);
      if (have_dfa && got != ose::dfa_match(dfa, s.data(), s.size())) {
        mismatches++;
        std::printf("NFA / DFA mismatch `%s` on random string %d\n", pattern.c_str(), k);
      }
    }
  }
  std::printf("patterns %llu strings %llu mismatches %llu\n", (unsigned long long)patterns, (unsigned long long)strings,
              (unsigned long long)mismatches);
  return mismatches ? 1 : 0;
}
