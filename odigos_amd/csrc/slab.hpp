// slab.hpp — one grow-only buffer carved into columns (HIP-free).  Every part
// starts on a 256-byte boundary and has at least 16 bytes of slack behind it:
// the kernels read 16-byte windows that may run past a column's end.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ose {

inline size_t up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// An offset cursor for the stage workspaces, which have no slack rule: take()
// rounds the cursor up to `align`, hands that offset out and moves past the
// part.  A layout function carves with it once; the bound and the pointers
// both come from the offsets it returns.
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes, size_t align = 256) {
    const size_t at = up(off, align);
    off = at + bytes;
    return at;
  }
};
// One part of a carved layout: byte offset from the layout's base, bytes.
struct WsPart { size_t off, bytes; };

struct SlabPart {
  void** dst;                  // takes base + the part's offset
  size_t bytes;
  const void* src = nullptr;   // host bytes for the staging copy, at the same offset
  bool staged = false;         // the caller fills the part in staging itself
};
// inputs: where the last sourced or staged part ends (the prefix that goes H2D)
struct SlabSize { size_t total = 0, inputs = 0; };

inline SlabSize slab_size(const std::vector<SlabPart>& parts) {
  size_t total = 0, inputs = 0;
  for (auto& p : parts) {
    total = up(total + p.bytes + 16);
    if (p.src || p.staged) inputs = total;
  }
  return {total, inputs};
}

// the parts' pointers into `base`, in the order given; with a staging base the
// sources are copied to their offsets there
inline void slab_assign(const std::vector<SlabPart>& parts, uint8_t* base, uint8_t* stage = nullptr) {
  size_t off = 0;
  for (auto& p : parts) {
    *p.dst = base + off;
    if (stage && p.src && p.bytes) std::memcpy(stage + off, p.src, p.bytes);
    off = up(off + p.bytes + 16);
  }
}

// Size, grow (buf to total, then the staging buffer to inputs), assign.  Buf:
// anything with `int need(size_t)` and `uint8_t* p`; a failing need() returns
// its code with no pointer touched.
template <class Buf, class Stage = Buf>
int slab_place(Buf& buf, const std::vector<SlabPart>& parts, Stage* stage = nullptr, SlabSize* size = nullptr) {
  const SlabSize z = slab_size(parts);
  int rc;
  if ((rc = buf.need(z.total)) || (stage && (rc = stage->need(z.inputs)))) return rc;
  slab_assign(parts, buf.p, stage ? stage->p : nullptr);
  if (size) *size = z;
  return 0;
}

}  // namespace ose
