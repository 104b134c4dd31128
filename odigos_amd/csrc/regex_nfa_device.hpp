// regex_nfa_device.hpp — regexp.MatchString by a bit-set simulation of the
// Thompson NFA (regex_nfa.hpp builds the tables), for the device
// (url_kernel.hip's NFA instances) and the host (osehost_regex_nfa_match, the
// sanitizer driver): one source.
//
// A state is a bit set over the M rune instructions: bit j = "rune
// instruction j was taken, the thread stands at its out".  Entry M is the
// start instruction, re-injected before every rune (unanchored search).  One
// step over a rune of class c whose EmptyOpContext with the previous rune is
// table x:
//   T  = union of succ[x][j] for j in S and j = M; a match bit among them
//        ends the match (MATCH is absorbing)
//   S' = T & in_class[c]
// and at the end of the text the match bits of context(prev, end of text)
// decide.  Equal to compile_dfa + dfa_match state for state: a DFA state is
// (S, type of the previous rune).
//
// The two bit sets live behind a Bits policy (at(k) / set(k, v), k < 2 *
// words): a plain array on the host, a slab column strided by the wave width
// on the device, so no runtime-indexed private array exists.
#pragma once
#include <cstdint>

#include "devcfg.hpp"

#if defined(__HIP__)
#define OSE_NFA_HD __host__ __device__ inline
#else
#define OSE_NFA_HD inline
#endif

namespace ose {
namespace nfa {

constexpr uint32_t kTypeBot = 0;   // rune types of regex_dfa.cpp's context()

// unicode/utf8.DecodeRune on [i, e): invalid -> (U+FFFD, 1)
template <class Reader>
OSE_NFA_HD uint32_t decode(Reader& rd, uint32_t i, uint32_t e, uint32_t& w) {
  const uint32_t c = rd.at(i);
  if (c < 0x80) { w = 1; return c; }
  uint32_t need, r, lo = 0x80, hi = 0xBF;
  if (c >= 0xC2 && c <= 0xDF) { need = 1; r = c & 0x1F; }
  else if (c == 0xE0) { need = 2; r = c & 0x0F; lo = 0xA0; }
  else if (c >= 0xE1 && c <= 0xEC) { need = 2; r = c & 0x0F; }
  else if (c == 0xED) { need = 2; r = c & 0x0F; hi = 0x9F; }
  else if (c >= 0xEE && c <= 0xEF) { need = 2; r = c & 0x0F; }
  else if (c == 0xF0) { need = 3; r = c & 0x07; lo = 0x90; }
  else if (c >= 0xF1 && c <= 0xF3) { need = 3; r = c & 0x07; }
  else if (c == 0xF4) { need = 3; r = c & 0x07; hi = 0x8F; }
  else { w = 1; return 0xFFFD; }
  if (i + need >= e) { w = 1; return 0xFFFD; }
  for (uint32_t k = 1; k <= need; k++) {
    const uint32_t b = rd.at(i + k);
    if (b < (k == 1 ? lo : 0x80u) || b > (k == 1 ? hi : 0xBFu)) { w = 1; return 0xFFFD; }
    r = (r << 6) | (b & 0x3F);
  }
  w = need + 1;
  return r;
}

// The tables of one program: `img` is the NfaDev, its offsets count from it.
struct View {
  const NfaDev* h;
  const uint8_t* img;
  OSE_NFA_HD const uint32_t* u32(uint32_t off) const { return reinterpret_cast<const uint32_t*>(img + off); }
  OSE_NFA_HD uint32_t cls(uint32_t r) const {
    if (r < 0x80) return h->ascii[r];
    const uint32_t* hr = u32(h->hi_off);
    uint32_t lo = 0, hi = h->hi_n;
    while (lo < hi) {
      const uint32_t m = (lo + hi) >> 1;
      if (r < hr[3 * m]) hi = m;
      else if (r > hr[3 * m + 1]) lo = m + 1;
      else return hr[3 * m + 2];
    }
    return 0;
  }
};

// The successors of entry j under context table x into T (bits words..2 *
// words - 1); true: the closure holds MATCH.
template <class Bits>
OSE_NFA_HD bool add_entry(const View& v, uint32_t x, uint32_t j, Bits& b) {
  const uint32_t m = v.h->m, words = v.h->words;
  const uint32_t* mt = v.u32(v.h->match_off) + x * ((m + 32) >> 5);
  if ((mt[j >> 5] >> (j & 31)) & 1u) return true;
  const uint32_t* row = v.u32(v.h->row_off) + x * (m + 2);
  const uint32_t* succ = v.u32(v.h->succ_off);
  for (uint32_t k = row[j]; k < row[j + 1]; k++) {
    const uint32_t t = succ[k];
    b.set(words + (t >> 5), b.at(words + (t >> 5)) | (1u << (t & 31)));
  }
  return false;
}

// T of the state S (bits 0..words - 1) and the start under context table x;
// true: a match.
template <class Bits>
OSE_NFA_HD bool gather(const View& v, uint32_t x, Bits& b) {
  const uint32_t m = v.h->m, words = v.h->words;
  for (uint32_t w = 0; w < words; w++) b.set(words + w, 0u);
  if (add_entry(v, x, m, b)) return true;
  for (uint32_t w = 0; w < words; w++) {
    uint32_t s = b.at(w);
    while (s) {
      const uint32_t j = (w << 5) + (uint32_t)__builtin_ctz(s);
      s &= s - 1;
      if (add_entry(v, x, j, b)) return true;
    }
  }
  return false;
}

// regexp.MatchString over bytes [s, e) of rd.  `b` holds 2 * words words.
template <class Reader, class Bits>
OSE_NFA_HD bool match(const uint8_t* img, Reader& rd, uint32_t s, uint32_t e, Bits& b) {
  const View v{reinterpret_cast<const NfaDev*>(img), img};
  const uint32_t words = v.h->words;
  const uint8_t* cls_type = img + v.h->cls_type_off;
  const uint32_t* in_class = v.u32(v.h->in_class_off);
  for (uint32_t w = 0; w < words; w++) b.set(w, 0u);
  uint32_t prev = kTypeBot;
  uint32_t i = s;
  while (i < e) {
    uint32_t wd;
    const uint32_t r = decode(rd, i, e, wd);
    i += wd;
    const uint32_t c = v.cls(r);
    const uint32_t t = cls_type[c];
    if (gather(v, v.h->ctx_of[prev * 4 + t], b)) return true;
    const uint32_t* ic = in_class + (uint64_t)c * words;
    for (uint32_t w = 0; w < words; w++) b.set(w, b.at(words + w) & ic[w]);
    prev = t;
  }
  return gather(v, v.h->ctx_of[prev * 4 + kTypeBot], b);
}

}  // namespace nfa
}  // namespace ose
