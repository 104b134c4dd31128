// Host check of slab.hpp's carver on fake buffers: every part at the offset
// the rule gives (256-byte starts, 16 bytes of slack behind each part, zero-byte
// parts included), total and inputs, the staging copies, a failing need();
// and the byte offsets of the groupbytrace store's control words
// (gbt_layout.hpp, HIP-free like slab.hpp).  Run by test_slab.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../odigos_amd/csrc/gbt_layout.hpp"
#include "../odigos_amd/csrc/slab.hpp"

namespace {
struct FakeBuf {   // grow-only, 512 bytes of 0xEE past what was asked for
  uint8_t* p = nullptr;
  std::vector<uint8_t> v;
  size_t asked = ~size_t(0);
  int need(size_t bytes) {
    asked = bytes;
    if (bytes + 512 > v.size()) v.assign(bytes + 512, 0xEE);
    p = v.data();
    return 0;
  }
};
struct OtherBuf : FakeBuf {};   // a second buffer type for the staging side
struct FailBuf {
  uint8_t* p = nullptr;
  int need(size_t) { return 7; }
};

int bad(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}
}  // namespace

int main() {
  using namespace ose;
  if (up(0) != 0 || up(1) != 256 || up(256) != 256 || up(257) != 512 || up(17, 16) != 32) return bad("up");

  // the stage workspaces' cursor: a part starts at the cursor rounded up to
  // its alignment and the cursor moves past it, with no slack and no rounding
  // behind the last part
  {
    Carve c;
    if (c.take(0) != 0 || c.off != 0) return bad("Carve: a zero-byte part at 0");
    if (c.take(40) != 0 || c.off != 40) return bad("Carve: the first part");
    if (c.take(8, 8) != 40 || c.off != 48) return bad("Carve: already on the alignment");
    if (c.take(3, 4) != 48 || c.off != 51) return bad("Carve: an odd size");
    if (c.take(4, 4) != 52 || c.off != 56) return bad("Carve: rounded up to 4");
    if (c.take(0) != 256 || c.off != 256) return bad("Carve: a zero-byte part moves the cursor to its alignment only");
    if (c.take(256) != 256 || c.off != 512) return bad("Carve: exactly one unit");
    if (c.take(257) != 512 || c.off != 769) return bad("Carve: one past a unit");
    if (c.take(1, 1) != 769 || c.off != 770) return bad("Carve: alignment 1");
    if (c.take(16) != 1024 || c.off != 1040) return bad("Carve: the default alignment is 256");
    Carve d{256};   // a cursor that starts past a header
    if (d.take(8 * 5) != 256 || d.take(4 * 5) != 512 || d.off != 532) return bad("Carve: started at 256");
  }

  // the groupbytrace store's control words (gbt_layout.hpp), where gbt_kernel.hip
  // and the scan and sort kernels have always been handed them
  {
    GbtWords w;
    const uint8_t* base = reinterpret_cast<const uint8_t*>(&w);
    const void* at[] = {&w.error, &w.totals[0], &w.totals[1], &w.worker_total, &w.scan_counter, &w.sort_gate,
                        &w.hdr_total, &w.total64, &w.status[0]};
    const size_t want[] = {0, 4, 8, 12, 16, 32, 36, 40, 64};
    for (size_t k = 0; k < 9; k++)
      if (static_cast<const uint8_t*>(at[k]) != base + want[k]) return bad("GbtWords: a member's offset");
    if (kGbtWordsError != 4 || kGbtWordsCount != 8 || kGbtWordsTotals != 12 || kGbtWordsScans != 16 ||
        kGbtWordsAll != 48 || kGbtWordsOtlp != 12)
      return bad("GbtWords: a cleared or read-back prefix");
  }

  // bytes, kind (0 device-only, 1 sourced, 2 staged by the caller), and the
  // offset worked out by hand
  struct Row { size_t bytes; int kind; size_t at; };
  const Row rows[] = {
      {0, 0, 0},         // zero bytes first: still 16 bytes of slack -> 256
      {1, 1, 256},       // 256 + 1 + 16 -> 512
      {240, 2, 512},     // 512 + 240 + 16 = 768: exactly on the boundary
      {241, 1, 768},     // 768 + 241 + 16 = 1025: one past it -> 1280
      {0, 0, 1280},      // zero bytes in the middle -> 1536
      {1000, 0, 1536},   // 1536 + 1016 = 2552 -> 2560
      {300, 1, 2560},    // the last input: 2560 + 316 = 2876 -> 3072
      {77, 0, 3072},     // 3072 + 93 = 3165 -> 3328
      {0, 0, 3328},      // zero bytes last -> 3584
  };
  const size_t kN = sizeof(rows) / sizeof(rows[0]), kTotal = 3584, kInputs = 3072;
  std::vector<std::vector<uint8_t>> src(kN);
  uint8_t marker = 0;
  std::vector<void*> dst(kN, &marker);
  std::vector<SlabPart> parts;
  for (size_t k = 0; k < kN; k++) {
    src[k].resize(rows[k].bytes);
    for (size_t q = 0; q < src[k].size(); q++) src[k][q] = (uint8_t)(1 + (k * 37 + q * 11) % 199);   // never 0xEE
    parts.push_back({&dst[k], rows[k].bytes, rows[k].kind == 1 ? src[k].data() : nullptr, rows[k].kind == 2});
  }
  // the rule, written out again: a part starts where the last one ended, and
  // ends at the next multiple of 256 at or after its bytes + 16
  size_t off = 0, inputs = 0;
  for (size_t k = 0; k < kN; k++) {
    if (off != rows[k].at) return bad("the hand-worked offsets do not follow the rule");
    off = (off + rows[k].bytes + 16 + 255) & ~size_t(255);
    if (rows[k].kind) inputs = off;
  }
  if (off != kTotal || inputs != kInputs) return bad("the hand-worked total / inputs do not follow the rule");

  const SlabSize z = slab_size(parts);
  if (z.total != kTotal || z.inputs != kInputs) return bad("slab_size");
  for (size_t k = 0; k < kN; k++)
    if (dst[k] != &marker) return bad("slab_size touched a destination");

  // a failing need(), of the buffer or of the staging buffer: its code, no pointer touched
  FailBuf fb;
  FakeBuf okb;
  if (slab_place(fb, parts) != 7 || slab_place(okb, parts, &fb) != 7) return bad("a failing need() must return its code");
  for (size_t k = 0; k < kN; k++)
    if (dst[k] != &marker) return bad("a failing need() left a destination changed");

  FakeBuf buf;
  OtherBuf stage;
  SlabSize got;
  if (slab_place(buf, parts, &stage, &got) != 0) return bad("slab_place");
  if (got.total != z.total || got.inputs != z.inputs) return bad("slab_place's size differs from slab_size's");
  if (buf.asked != kTotal || stage.asked != kInputs) return bad("need() was not asked for total / inputs");
  for (size_t k = 0; k < kN; k++)
    if (dst[k] != buf.p + rows[k].at) return bad("a destination is not at its offset");
  // staging: the sources byte for byte at their offsets, nothing else written
  // (the caller's staged part, the gaps, everything from `inputs` on)
  std::vector<uint8_t> want(stage.v.size(), 0xEE);
  for (size_t k = 0; k < kN; k++)
    if (rows[k].kind == 1) std::copy(src[k].begin(), src[k].end(), want.begin() + rows[k].at);
  if (stage.v != want) return bad("staging bytes");
  for (uint8_t x : buf.v)
    if (x != 0xEE) return bad("the buffer itself was written");

  // without a staging buffer: pointers only; slab_assign alone gives the same
  std::vector<void*> first = dst;
  dst.assign(kN, &marker);
  if (slab_place(buf, parts) != 0 || dst != first) return bad("slab_place without staging");
  dst.assign(kN, &marker);
  slab_assign(parts, buf.p);
  if (dst != first) return bad("slab_assign");
  // an empty list
  FakeBuf none;
  if (slab_place(none, {}, &stage, &got) != 0 || got.total != 0 || got.inputs != 0 || none.asked != 0) return bad("empty list");
  std::puts("OK");
  return 0;
}
