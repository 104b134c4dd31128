// regex_nfa.cpp — the device image of an NFA program and its host matcher
// (see regex_nfa.hpp; compile_nfa is in regex_dfa.cpp).
#include "regex_nfa.hpp"

#include <cstring>

#include "regex_nfa_device.hpp"

namespace ose {

namespace {

struct Image {
  std::vector<uint8_t> b;
  template <typename T>
  uint32_t put(const T* p, size_t n) {
    while (b.size() % 16) b.push_back(0);
    const uint32_t off = (uint32_t)b.size();
    const uint8_t* s = reinterpret_cast<const uint8_t*>(p);
    b.insert(b.end(), s, s + n * sizeof(T));
    return off;
  }
};

struct HostBytes {
  const uint8_t* p;
  uint32_t at(uint32_t i) const { return p[i]; }
};
struct HostBits {
  uint32_t* w;
  uint32_t at(uint32_t k) const { return w[k]; }
  void set(uint32_t k, uint32_t v) { w[k] = v; }
};

}  // namespace

std::vector<uint8_t> nfa_image(const NfaProgram& p) {
  Image im;
  NfaDev h{};
  h.m = p.m;
  h.words = p.words();
  h.nclasses = p.nclasses;
  h.nctx = p.nctx;
  h.hi_n = (uint32_t)p.hi_lo.size();
  std::memcpy(h.ctx_of, p.ctx_of, sizeof h.ctx_of);
  std::memcpy(h.ascii, p.ascii, sizeof h.ascii);
  im.put(&h, 1);
  std::vector<uint32_t> hr;
  for (size_t k = 0; k < p.hi_lo.size(); k++) { hr.push_back(p.hi_lo[k]); hr.push_back(p.hi_hi[k]); hr.push_back(p.hi_cls[k]); }
  h.hi_off = im.put(hr.data(), hr.size());
  h.row_off = im.put(p.row.data(), p.row.size());
  h.succ_off = im.put(p.succ.data(), p.succ.size());
  h.match_off = im.put(p.match.data(), p.match.size());
  h.in_class_off = im.put(p.in_class.data(), p.in_class.size());
  h.cls_type_off = im.put(p.cls_type.data(), p.cls_type.size());
  while (im.b.size() % 16) im.b.push_back(0);
  h.total_bytes = (uint32_t)im.b.size();
  std::memcpy(im.b.data(), &h, sizeof h);
  return std::move(im.b);
}

bool nfa_match(const std::vector<uint8_t>& image, const uint8_t* s, size_t n) {
  const NfaDev* h = reinterpret_cast<const NfaDev*>(image.data());
  std::vector<uint32_t> sets(2 * (size_t)h->words);
  HostBytes rd{s};
  HostBits bits{sets.data()};
  return nfa::match(image.data(), rd, 0u, (uint32_t)n, bits);
}

}  // namespace ose
