// gbt_layout.hpp — the groupbytrace store's device layouts (HIP-free): its
// control words and one layout function per scratch buffer.  gbt_host.cpp
// takes both the bytes it reserves and the pointers it hands the kernels from
// these, and osehost_gbt_layout shows them to tests/test_gbt_host_layout.py.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "slab.hpp"

namespace ose {

// The control words at the start of Gbt::words.  An add or a release clears
// [error, scan_counter), an OTLP add also [hdr_total, total64]; a read-back
// copies a prefix (kGbtRead*) into a host GbtWords.
struct GbtWords {
  uint32_t error;          // kGbtErr* bits (kernels.hpp), or a scan's or the sort's error
  uint32_t totals[2];      // the two scan totals: [0] new traces, released spans, then fragments; [1] string bytes
  uint32_t worker_total;   // the worker scan's total (number_workers; never read back)
  uint32_t scan_counter;   // the look-back scan's tile counter
  uint32_t pad0[3];
  uint32_t sort_gate;      // the sort kernels run while it is not 0 (opened with a 0x01 byte fill)
  uint32_t hdr_total;      // OTLP: the header-length scan's total
  uint64_t total64;        // OTLP: the call's bytes in 64 bits (GbtOtlp::total64)
  uint32_t pad1[4];
  uint64_t status[1];      // the look-back status, 8 bytes per scan tile, to the buffer's end
};
static_assert(offsetof(GbtWords, error) == 0, "GbtWords::error");
static_assert(offsetof(GbtWords, totals) == 4, "GbtWords::totals[0]");
static_assert(offsetof(GbtWords, totals) + sizeof(uint32_t) == 8, "GbtWords::totals[1]");
static_assert(offsetof(GbtWords, worker_total) == 12, "GbtWords::worker_total");
static_assert(offsetof(GbtWords, scan_counter) == 16, "GbtWords::scan_counter");
static_assert(offsetof(GbtWords, sort_gate) == 32, "GbtWords::sort_gate");
static_assert(offsetof(GbtWords, hdr_total) == 36, "GbtWords::hdr_total");
static_assert(offsetof(GbtWords, total64) == 40, "GbtWords::total64");
static_assert(offsetof(GbtWords, status) == 64, "GbtWords::status");
// the prefixes that are cleared and read back: the error word; with totals[0];
// with both totals; with worker_total; through total64.  And hdr_total with total64.
constexpr size_t kGbtWordsError = offsetof(GbtWords, totals), kGbtWordsCount = kGbtWordsError + sizeof(uint32_t),
                 kGbtWordsTotals = offsetof(GbtWords, worker_total), kGbtWordsScans = offsetof(GbtWords, scan_counter),
                 kGbtWordsAll = offsetof(GbtWords, pad1);
constexpr size_t kGbtWordsOtlp = offsetof(GbtWords, pad1) - offsetof(GbtWords, hdr_total);

// The scratch parts start on 256-byte boundaries.  All but the two u64 count
// arrays (slot_of, wcnt) carry 16 bytes of slack inside their extent: a part
// of 4n bytes takes up(4n + 16), not up(4n) + 16.  `end` is what to reserve.
inline WsPart gbt_part(Carve& c, size_t bytes, size_t slack = 16) { return WsPart{c.take(bytes + slack), bytes + slack}; }
inline WsPart gbt_no_part(Carve& c) { return WsPart{c.take(0), 0}; }   // a part this store does not have

// ose_gbt_add's scratch for n spans, A attribute sets, S scopes, R resources:
// slot_of (u64), flag, rank, strlen, stroff, the attribute-set map; W > 1: the
// (worker, rank) pairs; OTLP: the scopes' header lengths (two parts, sum,
// scan) and the staged ResourceSpans / ScopeSpans refs (u64)
struct GbtAddLayout {
  WsPart slot_of, flag, rank, strlen, stroff, attrset_map, keys, vals, hres, hscope, hlen, hoff, res_ref, scope_ref;
  size_t end;
};
inline GbtAddLayout gbt_add_layout(uint64_t n, uint64_t A, uint64_t S, uint64_t R, bool workers, bool otlp) {
  Carve c;
  GbtAddLayout L;
  L.slot_of = gbt_part(c, 8 * n, 0);
  L.flag = gbt_part(c, 4 * n);
  L.rank = gbt_part(c, 4 * n);
  L.strlen = gbt_part(c, 4 * n);
  L.stroff = gbt_part(c, 4 * n);
  L.attrset_map = gbt_part(c, 4 * A);
  L.keys = workers ? gbt_part(c, 4 * n) : gbt_no_part(c);
  L.vals = workers ? gbt_part(c, 4 * n) : gbt_no_part(c);
  L.hres = otlp ? gbt_part(c, 4 * S) : gbt_no_part(c);
  L.hscope = otlp ? gbt_part(c, 4 * S) : gbt_no_part(c);
  L.hlen = otlp ? gbt_part(c, 4 * S) : gbt_no_part(c);
  L.hoff = otlp ? gbt_part(c, 4 * S) : gbt_no_part(c);
  L.res_ref = otlp ? gbt_part(c, 8 * R) : gbt_no_part(c);
  L.scope_ref = otlp ? gbt_part(c, 8 * S) : gbt_no_part(c);
  L.end = up(c.off);
  return L;
}

// ose_gbt_release's scratch for a window of w pool spans
struct GbtReleaseLayout { WsPart flag, rank, strlen, stroff, keys, vals; size_t end; };
inline GbtReleaseLayout gbt_release_layout(uint64_t w) {
  Carve c;
  GbtReleaseLayout L;
  for (WsPart* p : {&L.flag, &L.rank, &L.strlen, &L.stroff, &L.keys, &L.vals}) *p = gbt_part(c, 4 * w);
  L.end = up(c.off);
  return L;
}

// the sort's ping-pong pairs and digit histograms: m pairs in T sort tiles
struct GbtSortLayout { WsPart k2, k3, v2, v3, hist, hoff; size_t end; };
inline GbtSortLayout gbt_sort_layout(uint64_t m, uint64_t T) {
  Carve c;
  GbtSortLayout L;
  for (WsPart* p : {&L.k2, &L.k3, &L.v2, &L.v3}) *p = gbt_part(c, 4 * m);
  for (WsPart* p : {&L.hist, &L.hoff}) *p = gbt_part(c, 4 * 256 * T);
  L.end = up(c.off);
  return L;
}

// the rings' OTLP columns (GbtOtlp): per pool slot, per scope slot
struct GbtOtlpRingLayout { WsPart msg_len, hdr_off, hdr_res, hdr_scope; size_t end; };
inline GbtOtlpRingLayout gbt_otlp_ring_layout(uint64_t pool_cap, uint64_t scope_cap) {
  Carve c;
  GbtOtlpRingLayout L;
  L.msg_len = gbt_part(c, 4 * pool_cap);
  L.hdr_off = gbt_part(c, 8 * scope_cap);
  L.hdr_res = gbt_part(c, 4 * scope_cap);
  L.hdr_scope = gbt_part(c, 4 * scope_cap);
  L.end = up(c.off);
  return L;
}

// num_workers W > 1 (Gbt::wdev): the workers' counts (u64), the batch's creators per worker, their scan
struct GbtWorkerLayout { WsPart wcnt, wadd, wstart; size_t end; };
inline GbtWorkerLayout gbt_worker_layout(uint64_t W) {
  Carve c;
  GbtWorkerLayout L;
  L.wcnt = gbt_part(c, 8 * W, 0);
  L.wadd = gbt_part(c, 4 * W);
  L.wstart = gbt_part(c, 4 * W);
  L.end = up(c.off);
  return L;
}

}  // namespace ose
