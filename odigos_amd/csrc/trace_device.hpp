// trace_device.hpp — device helpers shared by trace_kernel.hip (the sampling
// fast path), trace_slow_kernel.hip (run lists, the sort path) and
// shard_kernel.hip (the trace-id exchange).  Device-only, internal linkage,
// inlined into every caller: a kernel's machine code does not depend on the
// file it is compiled in.
//
// Latency monoid (latency.go:69-80): minStart is replaced when it is 0 or the
// new start is smaller, so a span with start 0 resets it.  Element
// (f, m, e): f bit0 = contains a zero start, bit1 = contains a span of the
// service; m = min start after the last zero start (+inf if none); e = max
// end.  later∘earlier = {f_a|f_b, b.reset ? b.m : min(a.m, b.m), max}.  The
// final minStart is m, or 0 when m = +inf.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "devcfg.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace ose {
namespace {

// Owner-side record columns (ose_shard_unpack): status bit 7 says the
// record's latency element begins with a zero start (a reset of minStart
// before its min start), include/odigos_amd.h "trace-id exchange".
constexpr uint32_t kStatusReset = 0x80u;
constexpr int kTWaves = 4;
constexpr int kTThreads = kTWaves * kWave;
constexpr int kSortThreads = 256;
constexpr uint64_t kInf = ~0ull;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t tid_hash(uint64_t hi, uint64_t lo) { return splitmix64(hi ^ splitmix64(lo)); }

// include/odigos_amd.h "injected randomness"
__device__ __forceinline__ double trace_uniform(uint64_t hi, uint64_t lo, uint64_t seed) {
  const uint64_t x = hi ^ ((lo << 29) | (lo >> 35)) ^ seed;
  return (double)(splitmix64(x) >> 11) * 0x1.0p-53;
}

__device__ __forceinline__ uint64_t lanemask_lt(int lane) { return (1ull << lane) - 1; }
__device__ __forceinline__ uint64_t lanemask_le(int lane) { return lane == 63 ? ~0ull : ((2ull << lane) - 1); }
__device__ __forceinline__ int ffs64(uint64_t x) { return __ffsll((unsigned long long)x) - 1; }
__device__ __forceinline__ int fls64(uint64_t x) { return 63 - __clzll((long long)x); }

// ---- DPP segmented scans ------------------------------------------------------
// Inclusive scans over the wave in lane order with (head, value) elements:
// earlier ⊕ later = (h_e | h_l, h_l ? v_l : v_e ∘ v_l).  row_shr 1/2/4/8 scan
// each 16-lane row, row_bcast:15 and :31 carry the row totals (the pattern of
// wave_incl_sum_u32); a source lane outside the row yields the identity.
// Register-only: no ds_bpermute round trip per step.
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_or_id(uint32_t x) { return dpp_mov<CTRL, ROWS>(0u, x); }
template <int CTRL, int ROWS>
__device__ __forceinline__ uint64_t dpp_or_id(uint64_t x) { return dpp_mov64<CTRL, ROWS>(0ull, x); }
// One step over any number of 32- and 64-bit words: every word's DPP move
// before the first OR (word by word costs the 128-VGPR kernels a register)
template <int CTRL, int ROWS, class... T>
__device__ __forceinline__ void seg_or_step(uint32_t& h, T&... v) {
  const uint32_t oh = dpp_mov<CTRL, ROWS>(0u, h);
  [&](auto... o) { if (!h) ((v |= o), ...); }(dpp_or_id<CTRL, ROWS>(v)...);
  h |= oh;
}
template <class... T>
__device__ __forceinline__ void seg_or_scan(uint32_t h, T&... v) {
  seg_or_step<0x111, 0xF>(h, v...);
  seg_or_step<0x112, 0xF>(h, v...);
  seg_or_step<0x114, 0xF>(h, v...);
  seg_or_step<0x118, 0xF>(h, v...);
  seg_or_step<0x142, 0xA>(h, v...);
  seg_or_step<0x143, 0xC>(h, v...);
}

// OR over the wave, broadcast: DPP row_shr within each 16-lane row, then the
// four row results read out (no ds_bpermute round trips)
__device__ __forceinline__ uint64_t wave_or64(uint64_t v) {
  v |= dpp_mov64<0x111, 0xF>(0ull, v);
  v |= dpp_mov64<0x112, 0xF>(0ull, v);
  v |= dpp_mov64<0x114, 0xF>(0ull, v);
  v |= dpp_mov64<0x118, 0xF>(0ull, v);
  return lane_value64(v, 15) | lane_value64(v, 31) | lane_value64(v, 47) | lane_value64(v, 63);
}

struct Cfg {
  const SampCfgDev* h;
  const SampRuleDev* rules;
  const SampLatDev* lat;
  const uint32_t* svc_slot;
  const uint64_t* slot_rules;
  const uint64_t* svc_bits;
  const uint8_t* bytes;
};
// the bytes of a rule table a kernel copies into LDS: a table longer than
// kSampCfgLds is one whose route bytes spill (one rule with a very long
// http_route: build_sampling_tables); the endpoint bits of such a chunk come
// precomputed (endpoint_plane_kernel), so its route bytes are never read
// from the LDS copy
__device__ __forceinline__ uint32_t cfg_lds_copy_bytes(const uint8_t* g) {
  const uint32_t t = reinterpret_cast<const SampCfgDev*>(g)->total_bytes;
  return t < kSampCfgLds ? t : kSampCfgLds;
}
// a workgroup of THREADS threads copies a rule table into LDS (16 bytes per
// thread and round; returns the bytes copied); the caller places the barrier
template <int THREADS>
__device__ __forceinline__ uint32_t copy_cfg_to_lds(uint8_t* dst, const uint8_t* src) {
  const uint32_t nb = cfg_lds_copy_bytes(src);
  for (uint32_t k = threadIdx.x * 16; k < nb; k += THREADS * 16)
    *reinterpret_cast<uint4*>(dst + k) = *reinterpret_cast<const uint4*>(src + k);
  return nb;
}
__device__ __forceinline__ Cfg load_cfg(const uint8_t* b) {
  Cfg c;
  c.h = reinterpret_cast<const SampCfgDev*>(b);
  c.rules = reinterpret_cast<const SampRuleDev*>(b + c.h->rules_off);
  c.lat = reinterpret_cast<const SampLatDev*>(b + c.h->lat_off);
  c.svc_slot = reinterpret_cast<const uint32_t*>(b + c.h->svc_slot_off);
  c.slot_rules = reinterpret_cast<const uint64_t*>(b + c.h->slot_rules_off);
  c.svc_bits = reinterpret_cast<const uint64_t*>(b + c.h->svc_bits_off);
  c.bytes = b + c.h->bytes_off;
  return c;
}

// The span_attribute bits of span j under a rule chunk's tables: its rules'
// attr_match bits [attr_base, attr_base + n_attr) (one 64-bit window: a
// chunk holds at most 64 service + span_attribute bits; attr_match is
// word-major, `words` planes of `stride` spans), placed after the chunk's
// service-rule bits
__device__ __forceinline__ uint64_t chunk_attr_bits(const uint64_t* am, uint64_t stride, uint32_t words,
                                                    const SampCfgDev* h, uint64_t j) {
  const uint32_t b = h->attr_base, w0 = b >> 6, sh = b & 63, na = h->n_attr;
  if (!na) return 0;
  uint64_t x = am[(uint64_t)w0 * stride + j] >> sh;
  if (sh && w0 + 1 < words) x |= am[(uint64_t)(w0 + 1) * stride + j] << (64 - sh);
  return (na >= 64 ? x : x & ((1ull << na) - 1)) << h->attr_shift;
}

struct Lat {
  uint32_t f;
  uint64_t m, e;
};
__device__ __forceinline__ Lat lat_comb(const Lat& a, const Lat& b) {   // a earlier, b later
  Lat r;
  r.f = a.f | b.f;
  r.m = (b.f & 1u) ? b.m : (a.m < b.m ? a.m : b.m);
  r.e = a.e > b.e ? a.e : b.e;
  return r;
}
// The element of one span of a latency service (rst: an owner-side record
// whose element begins with a zero start, kStatusReset).  A macro: as an
// inlined function, in each form tried, it changes the register allocation
// of trace_eval_kernel, trace_multi_kernel and trace_long_kernel, which sit
// at the register edge (profiles/trace_split_isa.txt).
#define LAT_OF_SPAN(st, en, rst) \
  Lat { ((st) == 0 || (rst)) ? 3u : 2u, (st) == 0 ? kInf : (st), (en) }

template <int CTRL, int ROWS>
__device__ __forceinline__ void seg_lat_step(uint32_t& h, Lat& v) {
  const uint32_t oh = dpp_mov<CTRL, ROWS>(0u, h);
  Lat o;
  o.f = dpp_mov<CTRL, ROWS>(0u, v.f);
  o.m = dpp_mov64<CTRL, ROWS>(kInf, v.m);
  o.e = dpp_mov64<CTRL, ROWS>(0ull, v.e);
  if (!h) v = lat_comb(o, v);
  h |= oh;
}
__device__ __forceinline__ void seg_lat_scan(uint32_t h, Lat& v) {
  seg_lat_step<0x111, 0xF>(h, v);
  seg_lat_step<0x112, 0xF>(h, v);
  seg_lat_step<0x114, 0xF>(h, v);
  seg_lat_step<0x118, 0xF>(h, v);
  seg_lat_step<0x142, 0xA>(h, v);
  seg_lat_step<0x143, 0xC>(h, v);
}

// strings.HasPrefix(route, rule.HttpRoute) (latency.go:97-100)
__device__ __forceinline__ bool route_has_prefix(const uint8_t* arena, ose_strref r, const uint8_t* pre, uint32_t n) {
  if (r.len < n) return false;
  const uint8_t* s = arena + r.off;
  for (uint32_t k = 0; k < n; k++)
    if (s[k] != pre[k]) return false;
  return true;
}

// The first 16 bytes of a string at arena offset `off` with `len` bytes:
// one aligned dwordx4 load, a second only when the bytes cross into the next
// 16-byte chunk (never past the string's own last chunk: the arena contract
// pads allocations to 16 bytes), funnel-shifted with v_alignbyte.
__device__ __forceinline__ uint4 head16(const uint8_t* arena, uint32_t off, uint32_t len) {
  const uint8_t* b = arena + (off & ~15u);
  const uint4 c0 = *reinterpret_cast<const uint4*>(b);
  uint4 c1 = make_uint4(0, 0, 0, 0);
  const uint32_t o = off & 15u;
  if (o + (len < 16u ? len : 16u) > 16u) c1 = *reinterpret_cast<const uint4*>(b + 16);
  const uint32_t q = o >> 2, sh = o & 3u;
  const uint32_t d0 = c0.x, d1 = c0.y, d2 = c0.z, d3 = c0.w, d4 = c1.x, d5 = c1.y, d6 = c1.z, d7 = c1.w;
  auto pick = [&](uint32_t j0, uint32_t j1, uint32_t j2, uint32_t j3) {   // d[k + q] for q = 0..3
    return q == 0 ? j0 : q == 1 ? j1 : q == 2 ? j2 : j3;
  };
  const uint32_t e0 = pick(d0, d1, d2, d3), e1 = pick(d1, d2, d3, d4), e2 = pick(d2, d3, d4, d5),
                 e3 = pick(d3, d4, d5, d6), e4 = pick(d4, d5, d6, d7);
  return make_uint4(__builtin_amdgcn_alignbyte(e1, e0, sh), __builtin_amdgcn_alignbyte(e2, e1, sh),
                    __builtin_amdgcn_alignbyte(e3, e2, sh), __builtin_amdgcn_alignbyte(e4, e3, sh));
}

// Endpoint bits of one span: the latency rules of its service whose
// http_route prefixes the span's AsString(http.route) (strings.HasPrefix,
// latency.go:97-100): one 16-byte window of the route, compared under each
// rule's byte mask; prefixes longer than 16 bytes finish bytewise.
__device__ __forceinline__ uint64_t endpoint_bits_w(const Cfg& c, uint32_t slot, const uint8_t* arena, ose_strref rt,
                                                    const uint4 w) {
  uint64_t rules = c.slot_rules[slot], ep = 0;
  if (!rules || rt.len == 0) return 0;
  while (rules) {
    const int k = ffs64(rules);
    rules &= rules - 1;
    const SampLatDev& L = c.lat[k];
    if (rt.len < L.route_len) continue;
    const bool head_ok = ((w.x & L.msk[0]) == L.pre[0]) && ((w.y & L.msk[1]) == L.pre[1]) &&
                         ((w.z & L.msk[2]) == L.pre[2]) && ((w.w & L.msk[3]) == L.pre[3]);
    if (!head_ok) continue;
    if (L.route_len > 16) {
      ose_strref tail{rt.off + 16, rt.len - 16};
      if (!route_has_prefix(arena, tail, c.bytes + L.route_off + 16, L.route_len - 16)) continue;
    }
    ep |= 1ull << k;
  }
  return ep;
}
__device__ __forceinline__ uint64_t endpoint_bits(const Cfg& c, uint32_t slot, const uint8_t* arena, ose_strref rt) {
  if (rt.len == 0 || !c.slot_rules[slot]) return 0;
  return endpoint_bits_w(c, slot, arena, rt, head16(arena, rt.off, rt.len));
}

// Latency rules of `slot` that matched (endpoint found) and whose duration
// reaches the threshold.  Duration: maxEnd.AsTime().Sub(minStart.AsTime())
// .Milliseconds() — int64 ns difference saturated like time.Sub, truncated.
__device__ __forceinline__ uint64_t latency_satisfied(const Cfg& c, uint32_t slot, uint64_t ep, uint64_t m, uint64_t e) {
  uint64_t rules = c.slot_rules[slot] & ep;
  if (!rules) return 0;
  const int64_t t = (int64_t)e, u = (int64_t)(m == kInf ? 0 : m);
  int64_t d;
  if (__builtin_sub_overflow(t, u, &d)) d = t < u ? INT64_MIN : INT64_MAX;
  // d / 1e6 >= threshold  <=>  d >= threshold_ns (no 64-bit division)
  uint64_t sat = 0;
  while (rules) {
    const int r = ffs64(rules);
    rules &= rules - 1;
    const int64_t tn = c.lat[r].threshold_ns;
    if (tn != INT64_MAX && d >= tn) sat |= 1ull << r;
  }
  return sat;
}

// uniform (scalar) copies of a rule's fields: the rule table lives in LDS,
// so its fields arrive in vector registers although every lane reads the
// same rule; branching on the vector copy cost exec-mask bookkeeping per rule
__device__ __forceinline__ uint32_t sgpr(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ double sgpr(double x) {
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  return __builtin_bit_cast(double, (uint64_t)sgpr((uint32_t)b) | ((uint64_t)sgpr((uint32_t)(b >> 32)) << 32));
}

// ShouldSample's level walk (rule_engine.go:55-83) over evaluateLevel's fold
// (rule_engine.go:89-115).  level: 0..2 satisfied level, 3 min fallback, 4 none.
// Without branches on per-trace values (the lanes of a flush decide 64
// traces together): every level is folded, the first satisfied one is kept
// (the early return of ShouldSample), and the min fallback of the matched
// levels is only read when no level was satisfied.  The rule fields are
// scalar, so the per-type cases are scalar branches.
__device__ __forceinline__ void decide(const Cfg& c, uint32_t err, uint64_t ep, uint64_t lsat, uint64_t svc, double u,
                              uint8_t& keep, uint8_t& level, double& ratio_out) {
  bool have_min = false, done = false;
  double min_fb = 0, out_ratio = 100.0;
  uint32_t out_level = 4;
  for (int L = 0; L < 3; L++) {
    double ratio = 0;
    bool sat = false, matched = false, found_fb = false;
    const uint32_t k0 = sgpr(c.h->level_first[L]), k1 = sgpr(c.h->level_first[L + 1]);
    for (uint32_t k = k0; k < k1; k++) {
      const SampRuleDev& r = c.rules[k];
      const uint32_t type = sgpr(r.type), bit = sgpr(r.bit);
      bool mt, st;
      double p;
      if (type == kSampError) {            // error.go:29-44
        mt = true;
        st = err != 0;
        p = st ? 100.0 : sgpr(r.fallback);
      } else if (type == kSampLatency) {   // latency.go:84-95
        mt = (ep >> bit) & 1;
        st = mt & (((lsat >> bit) & 1) != 0);
        p = st ? 100.0 : (mt ? sgpr(r.fallback) : 0.0);
      } else {                             // servicename.go:35-51
        mt = st = (svc >> bit) & 1;
        p = st ? sgpr(r.ratio) : sgpr(r.fallback);
      }
      // evaluateLevel: satisfied rules raise the ratio to their max; matched
      // unsatisfied ones take the first fallback, then the min of fallbacks
      const double rmax = ratio > p ? ratio : p;
      const double rfb = found_fb ? (ratio < p ? ratio : p) : p;
      ratio = st ? rmax : (mt ? rfb : ratio);
      found_fb |= !st & mt;
      sat |= st;
      matched |= mt;
    }
    const bool take = sat & !done;
    out_level = take ? (uint32_t)L : out_level;
    out_ratio = take ? ratio : out_ratio;
    done |= sat;
    const bool upd = matched & (!have_min | (ratio < min_fb));
    min_fb = upd ? ratio : min_fb;
    have_min |= matched;
  }
  if (!done) {
    out_level = have_min ? 3u : 4u;
    out_ratio = have_min ? min_fb : 100.0;
  }
  level = (uint8_t)out_level;
  ratio_out = out_ratio;
  keep = out_level == 4 ? 1 : (u * 100 < out_ratio);
}

// ShouldSample's walk (decide()) split at rule-chunk boundaries: walk_chunk
// takes one chunk's rules (level order, config order) from the state s (the
// open level, its evaluateLevel accumulators, the min fallback of the closed
// levels) and leaves it there; walk_finish closes the remaining levels and
// decides.  Chunk by chunk it is decide() over the whole rule list.
__device__ __forceinline__ void walk_close(FoldState& s) {   // the end of evaluateLevel for level s.level
  if (s.flags & kFsSat) {
    s.flags = kFsDone | (s.flags & kFsHaveMin);
    return;
  }
  if ((s.flags & kFsMatched) && (!(s.flags & kFsHaveMin) || s.ratio < s.min_fb)) {
    s.min_fb = s.ratio;
    s.flags |= kFsHaveMin;
  }
  s.flags &= kFsHaveMin;
  s.ratio = 0;
  s.level++;
}
__device__ void walk_chunk(const Cfg& c, FoldState& s, uint32_t err, uint64_t ep, uint64_t lsat, uint64_t svc) {
  for (uint32_t L = 0; L < 3 && !(s.flags & kFsDone); L++) {
    const uint32_t k0 = c.h->level_first[L], k1 = c.h->level_first[L + 1];
    if (k0 == k1) continue;
    while (s.level < L && !(s.flags & kFsDone)) walk_close(s);
    if (s.flags & kFsDone) break;
    for (uint32_t k = k0; k < k1; k++) {
      const SampRuleDev& r = c.rules[k];
      bool mt, st;
      double p;
      if (r.type == kSampError) {
        mt = true;
        st = err != 0;
        p = st ? 100.0 : r.fallback;
      } else if (r.type == kSampLatency) {
        mt = (ep >> r.bit) & 1;
        st = mt && ((lsat >> r.bit) & 1);
        p = st ? 100.0 : (mt ? r.fallback : 0.0);
      } else {
        mt = st = (svc >> r.bit) & 1;
        p = st ? r.ratio : r.fallback;
      }
      if (st) {
        s.ratio = s.ratio > p ? s.ratio : p;
        s.flags |= kFsSat | kFsMatched;
      } else if (mt) {
        s.flags |= kFsMatched;
        if (!(s.flags & kFsFoundFb)) {
          s.ratio = p;
          s.flags |= kFsFoundFb;
        } else {
          s.ratio = s.ratio < p ? s.ratio : p;
        }
      }
    }
  }
}
// walk_chunk over the matched rules only (trace_multi_kernel: a chunk of at
// most 128 rules, SampWalkDev): an unmatched rule changes nothing, and a
// level is closed when a matched rule of a later level comes (or by the
// next chunk / walk_finish) — the same state as walk_chunk leaves
__device__ __forceinline__ void walk_sparse(const Cfg& c, const SampWalkDev& W, FoldState& s, uint32_t err, uint64_t ep,
                                            uint64_t lsat, uint64_t svc) {
  uint64_t m[2] = {W.err[0], W.err[1]};
  for (uint64_t b = ep; b; b &= b - 1) {
    const uint32_t r = W.lat_rule[ffs64(b)];
    m[r >> 6] |= 1ull << (r & 63);
  }
  for (uint64_t b = svc; b; b &= b - 1) {
    const int x = ffs64(b);
    m[0] |= W.svc[x][0];
    m[1] |= W.svc[x][1];
  }
  const uint32_t lf1 = c.h->level_first[1], lf2 = c.h->level_first[2];
  for (int w = 0; w < 2; w++) {
    for (uint64_t mm = m[w]; mm && !(s.flags & kFsDone); mm &= mm - 1) {
      const uint32_t k = (uint32_t)(w * 64 + ffs64(mm));
      const uint32_t L = (k >= lf1 ? 1u : 0u) + (k >= lf2 ? 1u : 0u);
      while (s.level < L && !(s.flags & kFsDone)) walk_close(s);
      if (s.flags & kFsDone) break;
      const SampRuleDev& r = c.rules[k];
      bool mt, st;
      double p;
      if (r.type == kSampError) {
        mt = true;
        st = err != 0;
        p = st ? 100.0 : r.fallback;
      } else if (r.type == kSampLatency) {
        mt = (ep >> r.bit) & 1;
        st = mt && ((lsat >> r.bit) & 1);
        p = st ? 100.0 : (mt ? r.fallback : 0.0);
      } else {
        mt = st = (svc >> r.bit) & 1;
        p = st ? r.ratio : r.fallback;
      }
      if (st) {
        s.ratio = s.ratio > p ? s.ratio : p;
        s.flags |= kFsSat | kFsMatched;
      } else if (mt) {
        s.flags |= kFsMatched;
        if (!(s.flags & kFsFoundFb)) {
          s.ratio = p;
          s.flags |= kFsFoundFb;
        } else {
          s.ratio = s.ratio < p ? s.ratio : p;
        }
      }
    }
  }
}
__device__ __forceinline__ void walk_finish(FoldState& s, double u, uint8_t& keep, uint8_t& level, double& ratio_out) {
  while (s.level < 3 && !(s.flags & kFsDone)) walk_close(s);
  if (s.flags & kFsDone) {
    level = (uint8_t)s.level;
    ratio_out = s.ratio;
    keep = u * 100 < s.ratio;
  } else if (s.flags & kFsHaveMin) {
    level = 3;
    ratio_out = s.min_fb;
    keep = u * 100 < s.min_fb;
  } else {
    level = 4;
    ratio_out = 100.0;
    keep = 1;
  }
}

// One chunk of a rule-chunked configuration in a pass per chunk: the walk
// resumed from and saved to the trace's FoldState (first: the trace's first
// span); the last pass decides.
__device__ void decide_chunk(const TraceKernelArgs& a, const Cfg& c, uint64_t first, uint32_t err, uint64_t ep,
                             uint64_t lsat, uint64_t svc, double u, uint8_t& keep, uint8_t& level, double& ratio_out) {
  FoldState s = a.fold_in ? a.fold_in[first] : FoldState{0.0, 0.0, 0u, 0u};
  walk_chunk(c, s, err, ep, lsat, svc);
  if (a.fold_out) {   // more chunks follow: save the walk (this pass's keep is rewritten by the last)
    a.fold_out[first] = s;
    keep = 1;
    level = 4;
    ratio_out = 100.0;
    return;
  }
  walk_finish(s, u, keep, level, ratio_out);
}
// decide() or, in a rule-chunked pass, decide_chunk(); first: the trace's
// first span in batch order (the FoldState index)
__device__ __forceinline__ void decide_at(const TraceKernelArgs& a, const Cfg& c, uint64_t first, uint32_t err,
                                          uint64_t ep, uint64_t lsat, uint64_t svc, double u, uint8_t& keep,
                                          uint8_t& level, double& ratio_out) {
  if (a.fold_in || a.fold_out)
    decide_chunk(a, c, first, err, ep, lsat, svc, u, keep, level, ratio_out);
  else
    decide(c, err, ep, lsat, svc, u, keep, level, ratio_out);
}

__device__ __forceinline__ void write_rec(const TraceKernelArgs& a, uint64_t pos, uint8_t keep, uint8_t level,
                                          double ratio) {
  if (a.mode == kTraceBatch && a.batch_keep) *a.batch_keep = keep;
  if (!a.rec) return;
  TraceRec r;
  r.first_span = a.mode == kTracePerm ? a.perm[pos] : (uint32_t)pos;
  r.keep = keep;
  r.level = level;
  r._p0 = r._p1 = 0;
  r.ratio = ratio;
  a.rec[pos] = r;
}

}  // namespace
}  // namespace ose
