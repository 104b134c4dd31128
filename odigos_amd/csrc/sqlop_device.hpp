// sqlop_device.hpp — DetectSQLOperationName (odigossqldboperationprocessor/
// processor.go:84-115) over a byte reader, for the device (sqlop_kernel.hip's
// general path) and the host (osehost_sqlop_detect): one source.
//
// The Go code trims the query with strings.TrimSpace (unicode.IsSpace from
// both ends, an invalid byte being RuneError of width 1 and no space), takes
// the bytes up to the first ' ', '\t' or '\n', upper-cases them with
// strings.ToUpper and compares with seven keywords.  The same decision in one
// forward walk:
//   p  = the first byte that does not begin a valid space rune
//   K  = the keyword the bytes at p spell: letters in either case, U+017F
//        (C5 BF) for S and U+0131 (C4 B1) for I — the only non-ASCII runes
//        ToUpper maps to an ASCII letter; an invalid byte becomes U+FFFD and
//        never matches
//   R  = what follows K: it begins with one of the three delimiters (the first
//        word ends there), or it is valid space runes only (TrimSpace removed
//        it; UTF-8 is self-synchronising, so the backward decode of a run of
//        valid runes cuts it where the forward one does)
// Every loop advances by at least one byte and is bounded by the length.
#pragma once
#include <cstdint>

#if defined(__HIP__)   // compiled as HIP (sqlop_kernel.hip); plain C++ elsewhere
#define OSE_SQLOP_HD __host__ __device__ inline
#else
#define OSE_SQLOP_HD inline
#endif

namespace ose {
namespace sqlop {

// OSE_SQLOP_* of odigos_amd.h (repeated: the header is plain C++ for the host seam)
enum : uint32_t { kNone = 0, kSelect = 1, kInsert = 2, kUpdate = 3, kDelete = 4, kCreate = 5, kDrop = 6, kAlter = 7 };

OSE_SQLOP_HD bool ascii_space(uint32_t b) { return b == 0x20u || (b - 0x09u) <= 4u; }   // \t \n \v \f \r ' '
OSE_SQLOP_HD bool delimiter(uint32_t b) { return b == 0x20u || b == 0x09u || b == 0x0Au; }   // extractFirstWord (:106-115)

// Bytes of the unicode.IsSpace rune starting at i (0: none starts there).
// The set: U+0009-000D, U+0020, U+0085, U+00A0, U+1680, U+2000-200A, U+2028,
// U+2029, U+202F, U+205F, U+3000; each has one valid encoding, matched here
// byte for byte, so an overlong or truncated form is no space.
template <class Reader>
OSE_SQLOP_HD uint32_t space_rune(Reader& rd, uint32_t i, uint32_t n) {
  const uint32_t b0 = rd.at(i);
  if (b0 < 0x80u) return ascii_space(b0) ? 1u : 0u;
  if (b0 == 0xC2u) {
    if (i + 2 > n) return 0;
    const uint32_t b1 = rd.at(i + 1);
    return (b1 == 0x85u || b1 == 0xA0u) ? 2u : 0u;
  }
  if (b0 < 0xE1u || b0 > 0xE3u || i + 3 > n) return 0;
  const uint32_t b1 = rd.at(i + 1), b2 = rd.at(i + 2);
  bool sp;
  if (b0 == 0xE1u) sp = b1 == 0x9Au && b2 == 0x80u;                                  // U+1680
  else if (b0 == 0xE3u) sp = b1 == 0x80u && b2 == 0x80u;                             // U+3000
  else if (b1 == 0x80u) sp = (b2 >= 0x80u && b2 <= 0x8Au) || b2 == 0xA8u || b2 == 0xA9u || b2 == 0xAFu;
  else sp = b1 == 0x81u && b2 == 0x9Fu;                                              // U+205F
  return sp ? 3u : 0u;
}

constexpr uint64_t word6(char a, char b, char c, char d, char e, char f) {
  return ((uint64_t)(uint8_t)a << 40) | ((uint64_t)(uint8_t)b << 32) | ((uint64_t)(uint8_t)c << 24) |
         ((uint64_t)(uint8_t)d << 16) | ((uint64_t)(uint8_t)e << 8) | (uint64_t)(uint8_t)f;
}

template <class Reader>
OSE_SQLOP_HD uint32_t detect(Reader& rd, uint32_t n) {
  uint32_t p = 0;
  while (p < n) {
    const uint32_t w = space_rune(rd, p, n);
    if (!w) break;
    p += w;
  }
  if (p >= n) return kNone;   // len(TrimSpace(query)) == 0
  // up to six letters at p, upper-cased, most significant first; end[k] = the
  // byte after k + 1 letters
  uint64_t w = 0;
  uint32_t cnt = 0, q = p, end4 = 0, end5 = 0, end6 = 0;
  uint64_t w4 = 0, w5 = 0;
  while (cnt < 6 && q < n) {
    const uint32_t b = rd.at(q);
    uint32_t c;
    if (((b & 0xDFu) - 0x41u) < 26u) {
      c = b & 0xDFu;
      q += 1;
    } else if ((b == 0xC5u || b == 0xC4u) && q + 1 < n) {
      const uint32_t b1 = rd.at(q + 1);
      if (b == 0xC5u && b1 == 0xBFu) c = 'S';        // U+017F
      else if (b == 0xC4u && b1 == 0xB1u) c = 'I';   // U+0131
      else break;
      q += 2;
    } else {
      break;
    }
    w = (w << 8) | c;
    cnt++;
    if (cnt == 4) w4 = w, end4 = q;
    if (cnt == 5) w5 = w, end5 = q;
    if (cnt == 6) end6 = q;
  }
  uint32_t op = kNone, r = 0;
  if (cnt == 6) {
    r = end6;
    if (w == word6('S', 'E', 'L', 'E', 'C', 'T')) op = kSelect;
    else if (w == word6('I', 'N', 'S', 'E', 'R', 'T')) op = kInsert;
    else if (w == word6('U', 'P', 'D', 'A', 'T', 'E')) op = kUpdate;
    else if (w == word6('D', 'E', 'L', 'E', 'T', 'E')) op = kDelete;
    else if (w == word6('C', 'R', 'E', 'A', 'T', 'E')) op = kCreate;
  }
  if (!op && cnt >= 5 && w5 == word6(0, 'A', 'L', 'T', 'E', 'R')) op = kAlter, r = end5;
  if (!op && cnt >= 4 && w4 == word6(0, 0, 'D', 'R', 'O', 'P')) op = kDrop, r = end4;
  if (!op) return kNone;
  if (r >= n) return op;
  if (delimiter(rd.at(r))) return op;
  while (r < n) {
    const uint32_t sw = space_rune(rd, r, n);
    if (!sw) return kNone;
    r += sw;
  }
  return op;
}

// plain bytes in host memory
struct HostBytes {
  const uint8_t* p;
  OSE_SQLOP_HD uint32_t at(uint32_t i) const { return p[i]; }
};

}  // namespace sqlop
}  // namespace ose
