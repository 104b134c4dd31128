// url_full.hpp — net/url.Parse(rawURL).Path over bytes read in place, for the
// host and the device alike (engine option otlp_url_full).
//
// urlparse.cpp's go_url_parse_path restated without a string: the same
// grammar (Parse's '#' cut and control-character check, "*", getScheme, the
// '?' cut, the opaque form, "first path segment cannot contain colon", the
// "//" authority rule, parseAuthority, parseHost, validOptionalPort,
// validUserinfo, unescape's validity in each mode, setPath, setFragment) as
// index ranges over a byte source `src.at(offset)`: pbdev's ByteReader on
// the device (otlp_url_full_kernel.hip), a string_view on the host
// (osehost_url_full_parse, tests/url_full_check.cpp).  Of the authority, the
// userinfo and the fragment only the validity is computed; nothing but the
// Path is ever produced, and the Path is a sub-range of the input unless it
// holds escapes.  HIP-free: plain g++ compiles it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OSE_UF_FN __host__ __device__ inline
#else
#define OSE_UF_FN inline
#endif

namespace ose {
namespace urlfull {

enum Outcome : uint32_t {
  kError = 0,     // url.Parse returns an error
  kEmpty = 1,     // ok, Path ""
  kInPlace = 2,   // ok, Path = [off, off + len) of the input
  kDecoded = 3,   // ok, the path part [off, off + len) holds escapes; dec_len bytes once unescaped
};
struct Result {
  uint32_t outcome, off, len, dec_len;
};

enum Mode : uint32_t { kPath, kHost, kZone, kUserPassword, kFragment };

OSE_UF_FN bool ishex(uint32_t c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'); }
OSE_UF_FN uint32_t unhex(uint32_t c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return c - 'A' + 10;
}
OSE_UF_FN bool isalnum_ascii(uint32_t c) {
  return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9');
}

// shouldEscape in the host and zone modes (the only modes unescape consults
// it in; the two agree on every byte)
OSE_UF_FN bool host_should_escape(uint32_t c) {
  if (isalnum_ascii(c)) return false;
  switch (c) {
    case '!': case '$': case '&': case '\'': case '(': case ')': case '*': case '+': case ',':
    case ';': case '=': case ':': case '[': case ']': case '<': case '>': case '"':
    case '-': case '_': case '.': case '~':
      return false;
  }
  return true;
}

// unescape's validity over [s, e); *escapes: the '%' it holds
template <class Src>
OSE_UF_FN bool unescape_ok(Src& src, uint32_t s, uint32_t e, Mode mode, uint32_t* escapes) {
  uint32_t n = 0;
  for (uint32_t i = s; i < e;) {
    const uint32_t c = src.at(i);
    if (c == '%') {
      n++;
      if (e - i <= 2) return false;
      const uint32_t h = src.at(i + 1), l = src.at(i + 2);
      if (!ishex(h) || !ishex(l)) return false;
      const bool pct = h == '2' && l == '5';   // "%25"
      if (mode == kHost && unhex(h) < 8 && !pct) return false;
      if (mode == kZone) {
        const uint32_t v = unhex(h) << 4 | unhex(l);
        if (!pct && v != ' ' && host_should_escape(v)) return false;
      }
      i += 3;
    } else {
      if ((mode == kHost || mode == kZone) && c < 0x80 && host_should_escape(c)) return false;
      i++;
    }
  }
  if (escapes) *escapes = n;
  return true;
}

constexpr uint32_t kNone = 0xFFFFFFFFu;
template <class Src>
OSE_UF_FN uint32_t find(Src& src, uint32_t s, uint32_t e, uint32_t c) {
  for (uint32_t i = s; i < e; i++)
    if (src.at(i) == c) return i;
  return kNone;
}
template <class Src>
OSE_UF_FN uint32_t rfind(Src& src, uint32_t s, uint32_t e, uint32_t c) {
  for (uint32_t i = e; i > s; i--)
    if (src.at(i - 1) == c) return i - 1;
  return kNone;
}

// validOptionalPort: "" or ":" and digits
template <class Src>
OSE_UF_FN bool valid_optional_port(Src& src, uint32_t s, uint32_t e) {
  if (s == e) return true;
  if (src.at(s) != ':') return false;
  for (uint32_t i = s + 1; i < e; i++) {
    const uint32_t c = src.at(i);
    if (c < '0' || c > '9') return false;
  }
  return true;
}

template <class Src>
OSE_UF_FN bool parse_host(Src& src, uint32_t s, uint32_t e) {
  if (s < e && src.at(s) == '[') {
    const uint32_t i = rfind(src, s, e, ']');
    if (i == kNone) return false;
    if (!valid_optional_port(src, i + 1, e)) return false;
    // the zone: the first "%25" before the ']'
    uint32_t zone = kNone;
    for (uint32_t z = s; z + 3 <= i; z++)
      if (src.at(z) == '%' && src.at(z + 1) == '2' && src.at(z + 2) == '5') { zone = z; break; }
    if (zone != kNone)
      return unescape_ok(src, s, zone, kHost, nullptr) && unescape_ok(src, zone, i, kZone, nullptr) &&
             unescape_ok(src, i, e, kHost, nullptr);
  } else {
    const uint32_t i = rfind(src, s, e, ':');
    if (i != kNone && !valid_optional_port(src, i, e)) return false;
  }
  return unescape_ok(src, s, e, kHost, nullptr);
}

// validUserinfo: RFC 3986 userinfo characters (only ASCII is checked)
template <class Src>
OSE_UF_FN bool valid_userinfo(Src& src, uint32_t s, uint32_t e) {
  for (uint32_t i = s; i < e; i++) {
    const uint32_t r = src.at(i);
    if (isalnum_ascii(r) || r >= 0x80) continue;
    switch (r) {
      case '-': case '.': case '_': case ':': case '~': case '!': case '$': case '&': case '\'':
      case '(': case ')': case '*': case '+': case ',': case ';': case '=': case '%': case '@':
        continue;
      default:
        return false;
    }
  }
  return true;
}

template <class Src>
OSE_UF_FN bool parse_authority(Src& src, uint32_t s, uint32_t e) {
  const uint32_t i = rfind(src, s, e, '@');
  if (!parse_host(src, i == kNone ? s : i + 1, e)) return false;
  if (i == kNone) return true;
  if (!valid_userinfo(src, s, i)) return false;
  const uint32_t c = find(src, s, i, ':');
  if (c == kNone) return unescape_ok(src, s, i, kUserPassword, nullptr);
  return unescape_ok(src, s, c, kUserPassword, nullptr) && unescape_ok(src, c + 1, i, kUserPassword, nullptr);
}

// url.Parse of bytes [off, off + len) of `src`
template <class Src>
OSE_UF_FN Result parse(Src& src, uint32_t off, uint32_t len) {
  const Result error{kError, 0, 0, 0};
  const uint32_t end = off + len;
  const uint32_t hash = find(src, off, end, '#');
  const uint32_t ue = hash == kNone ? end : hash;
  // parse(u, viaRequest=false)
  for (uint32_t i = off; i < ue; i++) {
    const uint32_t c = src.at(i);
    if (c < 0x20 || c == 0x7F) return error;   // invalid control character
  }
  Result out{kEmpty, off, 0, 0};
  bool opaque = false;
  if (ue - off == 1 && src.at(off) == '*') {
    out = Result{kInPlace, off, 1, 0};
  } else {
    // getScheme
    bool scheme = false;
    uint32_t rs = off, re = ue;
    for (uint32_t i = off; i < ue; i++) {
      const uint32_t c = src.at(i);
      if ((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z')) continue;
      if ((c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.') {
        if (i == off) break;
        continue;
      }
      if (c == ':') {
        if (i == off) return error;   // missing protocol scheme
        scheme = true;
        rs = i + 1;
      }
      break;
    }
    // the query goes (a lone trailing '?' is the first '?' too)
    const uint32_t q = find(src, rs, re, '?');
    if (q != kNone) re = q;
    if (rs == re || src.at(rs) != '/') {
      if (scheme) {
        opaque = true;   // opaque URL: Path stays ""
      } else {
        // first path segment cannot contain colon
        for (uint32_t i = rs; i < re; i++) {
          const uint32_t c = src.at(i);
          if (c == '/') break;
          if (c == ':') return error;
        }
      }
    }
    if (!opaque) {
      const bool two = re - rs >= 2 && src.at(rs) == '/' && src.at(rs + 1) == '/';
      const bool three = two && re - rs >= 3 && src.at(rs + 2) == '/';
      if ((scheme || !three) && two) {
        const uint32_t as = rs + 2;
        const uint32_t slash = find(src, as, re, '/');
        const uint32_t ae = slash == kNone ? re : slash;
        rs = ae;
        if (!parse_authority(src, as, ae)) return error;
      }
      uint32_t escapes = 0;
      if (!unescape_ok(src, rs, re, kPath, &escapes)) return error;   // setPath
      if (escapes) out = Result{kDecoded, rs, re - rs, re - rs - 2 * escapes};
      else if (re > rs) out = Result{kInPlace, rs, re - rs, 0};
      else out = Result{kEmpty, rs, 0, 0};
    }
  }
  if (hash != kNone && end - hash > 1)
    if (!unescape_ok(src, hash + 1, end, kFragment, nullptr)) return error;   // setFragment
  return out;
}

// the Path of a kDecoded result: [off, off + len) unescaped into out (dec_len bytes)
template <class Src>
OSE_UF_FN void unescape_into(Src& src, uint32_t off, uint32_t len, uint8_t* out) {
  const uint32_t e = off + len;
  for (uint32_t i = off; i < e;) {
    const uint32_t c = src.at(i);
    if (c == '%') {
      *out++ = (uint8_t)(unhex(src.at(i + 1)) << 4 | unhex(src.at(i + 2)));
      i += 3;
    } else {
      *out++ = (uint8_t)c;
      i++;
    }
  }
}

// the host's byte source
struct ViewSrc {
  const char* p;
  OSE_UF_FN uint32_t at(uint32_t i) const { return (uint8_t)p[i]; }
};

}  // namespace urlfull
}  // namespace ose
