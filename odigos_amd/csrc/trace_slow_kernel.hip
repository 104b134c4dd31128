// trace_slow_kernel.hip — the slow paths of odigossampling on CDNA4 (gfx950),
// taken when a batch repeats a trace id (the fast path of trace_kernel.hip
// set *dup), and the dense per-trace outputs.
//
// Run-list path (gated on *dup): trace_runs_kernel lists every run in its
// trace's slot of the exact trace-id table, trace_fold_kernel folds every
// trace of 2..kMaxRuns runs on one lane, trace_first_select_kernel keeps each
// trace's first head.  A trace past the fold's limits sets *overflow.
//
// Sort path (gated on the caller's gate word; the sampling stage passes
// *overflow): trace_key_kernel keys every span by its trace's first run-head
// position in the exact table, sort_hist_kernel / sort_scatter_kernel with
// scan_u32_kernel sort the spans by that key (stable LSD radix sort; the
// groupbytrace release sorts with the same kernels), and trace_eval_kernel
// (trace_kernel.hip) evaluates the sorted positions, every trace one run.
//
// Gating: each of these kernels reads its gate word first and returns when
// it is closed (a null gate is open), those of the sampling stage over a
// grid capped at kGatedBlocks.  trace_compact_kernel (records -> dense
// per-trace outputs) has no gate.  Shared device helpers: trace_device.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "trace_device.hpp"

namespace ose {
namespace {

__device__ __forceinline__ bool gated(const uint32_t* g) {
  return g && __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
}

// ---- exact trace_id table -------------------------------------------------
// Insert protocol: CAS the state from a stale epoch to BUSY, store the key
// with sc1 (agent-scope relaxed) stores, drain them (s_waitcnt vmcnt(0)), then
// store READY; readers poll the state and read the key with sc1 loads
// (MI355X_MICROARCH.md "Valid forms": sc1 payload + drained flag).  A lane
// that finds the key ready and equal is a second run of that trace_id.
// Returns kInsNew (the slot was claimed; with run lists, the run is listed
// as the trace's first), kInsFound (the id was there: a repeated trace id)
// or kInsFail (error flagged).  Callers gated on *dup do not set it again:
// one word hit by every repeated head of the batch is a serialised
// device-scope atomic per head.
constexpr int kInsNew = 0, kInsFound = 1, kInsFail = -1;
__device__ inline int table_insert(const TraceKernelArgs& a, uint64_t hi, uint64_t lo, uint32_t pos,
                                    uint64_t* slot_out = nullptr) {
  const uint32_t busy = (a.epoch << 2) | 1u, ready = (a.epoch << 2) | 2u;
  uint64_t h = tid_hash(hi, lo) & a.table_mask;
  uint32_t probes = 0, spins = 0;
  for (;;) {
    TraceSlot* s = &a.table[h];
    const uint32_t st = __hip_atomic_load(&s->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((st >> 2) != a.epoch) {
      uint32_t expect = st;
      if (__hip_atomic_compare_exchange_strong(&s->state, &expect, busy, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        __hip_atomic_store(&s->hi, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->lo, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->first, pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a.run_count) {   // this run is the trace's first listed run
          __hip_atomic_store(&a.run_count[h], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (a.runs) a.runs[h * kMaxRuns] = pos;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&s->state, ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (slot_out) *slot_out = h;
        return kInsNew;
      }
      continue;   // lost the race for this slot: look at it again
    }
    if ((st & 3u) != 2u) {   // another lane is publishing this slot
      if (++spins > (1u << 20)) {
        atomicOr(a.error, 1u);
        return kInsFail;
      }
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    const uint64_t h2 = __hip_atomic_load(&s->hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t l2 = __hip_atomic_load(&s->lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (h2 == hi && l2 == lo) {
      atomicMin(&s->first, pos);
      if (slot_out) *slot_out = h;
      return kInsFound;
    }
    h = (h + 1) & a.table_mask;
    if (++probes > a.table_mask) {
      atomicOr(a.error, 4u);
      return kInsFail;
    }
  }
}

// Every run head inserts its full trace id; a trace's entry keeps its
// smallest run-head position.  Gated kernels use a grid-stride loop over a
// capped grid: a closed launch (the common case) costs a few microseconds,
// not one block per 256 spans.
constexpr uint32_t kGatedBlocks = 2048;
__global__ __launch_bounds__(256) void trace_insert_exact_kernel(TraceKernelArgs a) {
  if (__hip_atomic_load(a.dup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < a.n_spans; p += (uint64_t)gridDim.x * 256) {
    const uint64_t hi = a.tid[2 * p], lo = a.tid[2 * p + 1];
    if (p > 0 && a.tid[2 * p - 2] == hi && a.tid[2 * p - 1] == lo) continue;
    (void)table_insert(a, hi, lo, (uint32_t)p);   // gated on *dup: already set
  }
}

// ---- run-list path ---------------------------------------------------------
// A batch with repeated trace ids (resource-shuffled input, or the records a
// trace's owner GPU receives from several sources) usually holds each trace
// in a few runs.  trace_runs_kernel inserts every run head (the window head
// masks of the fast pass) into the exact table and lists the run in the
// trace's slot; trace_fold_kernel then folds, for every trace with 2 or
// more runs, its runs in batch order on one lane (exactly the fold
// trace_eval_kernel does over a contiguous trace), decides and writes keep
// over all its runs.  Traces with more than kMaxRuns runs, more than
// kMaxFoldSpans spans or more than kMaxFoldSlots latency services set
// *overflow, and the sort-based path (gated on it) recomputes the batch.
__global__ __launch_bounds__(256) void trace_runs_kernel(TraceKernelArgs a) {
  if (__hip_atomic_load(a.dup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  if (a.path_count && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.path_count, 1ull);
  const int lane = threadIdx.x & 63;
  for (uint64_t w = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / kWave; w < a.n_windows;
       w += (uint64_t)gridDim.x * (256 / kWave)) {
    const uint64_t heads = a.win_heads[w];
    const uint64_t p = w * kWave + lane;
    if (!((heads >> lane) & 1) || p >= a.n_spans) continue;
    const uint64_t hi = a.tid[2 * p], lo = a.tid[2 * p + 1];
    uint64_t slot = ~0ull;
    const int ins = table_insert(a, hi, lo, (uint32_t)p, &slot);   // gated on *dup: not set again
    if (ins == kInsFail || slot == ~0ull) {   // table full / spin gave up: error already flagged
      atomicOr(a.overflow, 1u);
      continue;
    }
    if (ins == kInsFound) {   // a later run: append (the claiming lane listed the first)
      const uint32_t k = atomicAdd(&a.run_count[slot], 1u);
      if (k < kMaxRuns) a.runs[slot * kMaxRuns + k] = (uint32_t)p;
      else atomicOr(a.overflow, 1u);
    }
    a.head_slot[p] = (uint32_t)slot;
  }
}

// end of the run starting at head position p: the next head after it
__device__ __forceinline__ uint64_t run_end(const TraceKernelArgs& a, uint64_t p) {
  uint64_t w = p / kWave;
  uint64_t m = a.win_heads[w] & ~lanemask_le((int)(p % kWave));
  while (!m) {
    if (++w >= a.n_windows) return a.n_spans;
    m = a.win_heads[w];
  }
  return w * kWave + (uint64_t)ffs64(m);
}

__global__ __launch_bounds__(kTThreads) void trace_fold_kernel(TraceKernelArgs a) {
  if (__hip_atomic_load(a.dup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  // the sort-based path already has the batch (it redoes every trace)
  if (__hip_atomic_load(a.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
  __shared__ __attribute__((aligned(16))) uint8_t cfg_lds[kSampCfgLds];
  copy_cfg_to_lds<kTThreads>(cfg_lds, a.cfg);
  __syncthreads();
  const Cfg c = load_cfg(cfg_lds);
  const uint32_t nsvc = c.h->n_services;
  const bool want_route = c.h->n_lat && !a.route_match && a.route;
  const int lane = threadIdx.x & 63;
  for (uint64_t w = ((uint64_t)blockIdx.x * kTThreads + threadIdx.x) / kWave; w < a.n_windows;
       w += (uint64_t)gridDim.x * kTWaves) {
    const uint64_t heads = a.win_heads[w];
    const uint64_t p = w * kWave + lane;
    const bool head = ((heads >> lane) & 1) && p < a.n_spans;
    uint32_t slot = 0, nr = 0;
    bool first = false;
    if (head) {
      slot = a.head_slot[p];
      first = a.table[slot].first == (uint32_t)p;
      nr = __hip_atomic_load(&a.run_count[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint64_t fm = __ballot(first);
    if (lane == 0) a.win_first[w] = fm;
    if (!first || nr < 2 || nr > kMaxRuns) continue;   // one run: the fast pass decided it
    // the trace's runs in batch order
    uint32_t rs[kMaxRuns];
#pragma unroll
    for (uint32_t k = 0; k < kMaxRuns; k++) rs[k] = k < nr ? a.runs[(uint64_t)slot * kMaxRuns + k] : 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t k = 1; k < kMaxRuns; k++)   // insertion sort, unrolled (nr <= 8)
#pragma unroll
      for (uint32_t j = k; j > 0; j--)
        if (rs[j - 1] > rs[j]) { const uint32_t t = rs[j]; rs[j] = rs[j - 1]; rs[j - 1] = t; }
    uint32_t err = 0, nslots = 0;
    uint64_t ep = 0, svcb = 0, spans = 0;
    uint32_t ks[kMaxFoldSlots];
    Lat ls[kMaxFoldSlots];
    bool over = false;
    for (uint32_t r = 0; r < nr && !over; r++) {
      const uint64_t s0 = rs[r], s1 = run_end(a, s0);
      spans += s1 - s0;
      if (spans > kMaxFoldSpans) { over = true; break; }
      for (uint64_t q = s0; q < s1; q++) {
        const uint32_t res = a.resource[q], stt = a.status[q];
        err |= (stt & ~kStatusReset) == OSE_STATUS_ERROR;
        const uint32_t sv = a.res_svc[res];
        if (a.svc_match) {
          svcb |= a.svc_match[q];
        } else {
          const uint32_t ss = a.res_svc_str[res];
          if (ss < nsvc) svcb |= c.svc_bits[ss];
          if (a.attr_match) svcb |= chunk_attr_bits(a.attr_match, a.attr_stride, a.attr_words, c.h, q);
        }
        if (sv >= nsvc) continue;
        const uint32_t slt = c.svc_slot[sv];
        if (slt == kNoSlot) continue;
        ep |= a.route_match ? a.route_match[q] & c.slot_rules[slt]
                            : (want_route ? endpoint_bits(c, slt, a.arena, a.route[q]) : 0ull);
        const uint64_t st = a.start ? a.start[q] : 0, en = a.end ? a.end[q] : 0;
        const Lat v = LAT_OF_SPAN(st, en, stt & kStatusReset);
        uint32_t k = 0;
        while (k < nslots && ks[k] != slt) k++;
        if (k == nslots) {
          if (nslots == kMaxFoldSlots) { over = true; break; }
          ks[nslots] = slt;
          ls[nslots] = Lat{0u, kInf, 0ull};
          nslots++;
        }
        ls[k] = lat_comb(ls[k], v);
      }
    }
    if (over) {
      atomicOr(a.overflow, 1u);
      continue;
    }
    uint64_t lsat = 0;
    for (uint32_t k = 0; k < nslots; k++)
      if (ls[k].f & 2u) lsat |= latency_satisfied(c, ks[k], ep, ls[k].m, ls[k].e);
    const uint64_t hi = a.tid[2 * p], lo = a.tid[2 * p + 1];
    uint8_t dk = 0, dl = 0;
    double dr = 0;
    decide_at(a, c, p, err, ep, lsat, svcb, trace_uniform(hi, lo, a.seed), dk, dl, dr);
    write_rec(a, p, dk, dl, dr);
    for (uint32_t r = 0; r < nr; r++) {
      const uint64_t s0 = rs[r], s1 = run_end(a, s0);
      for (uint64_t q = s0; q < s1; q++) a.keep[q] = dk;
    }
  }
}

// the per-trace outputs list first runs only, unless the sort-based path
// (gated on *overflow) rewrites the head masks itself
__global__ __launch_bounds__(256) void trace_first_select_kernel(TraceKernelArgs a) {
  if (__hip_atomic_load(a.dup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  if (__hip_atomic_load(a.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
  for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < a.n_windows; w += (uint64_t)gridDim.x * 256)
    a.win_heads[w] = a.win_first[w];
}

// key[i] = first run-head position of span i's trace_id (read-only probe of
// the exact table).
__global__ __launch_bounds__(256) void trace_key_kernel(TraceSortArgs a) {
  if (gated(a.gate)) return;
  if (a.path_count && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.path_count + 1, 1ull);
  const uint32_t ready = (a.epoch << 2) | 2u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.n_spans; i += (uint64_t)gridDim.x * 256) {
    const uint64_t hi = a.tid[2 * i], lo = a.tid[2 * i + 1];
    uint64_t h = tid_hash(hi, lo) & a.table_mask;
    bool found = false;
    for (uint64_t probes = 0; probes <= a.table_mask; probes++) {
      const TraceSlot& s = a.table[h];
      if (s.state == ready && s.hi == hi && s.lo == lo) {
        a.key[i] = s.first;
        found = true;
        break;
      }
      if ((s.state >> 2) != a.epoch) break;
      h = (h + 1) & a.table_mask;
    }
    if (!found) {
      atomicOr(a.error, 4u);
      a.key[i] = 0;
    }
  }
}

constexpr int kSortRounds = kSortTile / kSortThreads;

__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(TraceSortArgs a) {
  if (gated(a.gate)) return;
  __shared__ uint32_t hist[256];
  const int t = threadIdx.x;
  if (a.scan_status) {
    for (uint32_t k = blockIdx.x * kSortThreads + t; k < a.scan_status_n; k += gridDim.x * kSortThreads)
      a.scan_status[k] = 0;
    if (blockIdx.x == 0 && t == 0) *a.scan_counter = 0;
  }
  hist[t] = 0;
  __syncthreads();
  const uint32_t* keys = a.keys_in ? a.keys_in : a.key;
  const uint64_t b = (uint64_t)blockIdx.x * kSortTile;
  for (int r = 0; r < kSortRounds; r++) {
    const uint64_t j = b + (uint64_t)r * kSortThreads + t;
    if (j < a.n_spans) atomicAdd(&hist[(keys[j] >> a.shift) & 255u], 1u);
  }
  __syncthreads();
  a.hist[(uint64_t)t * a.n_tiles + blockIdx.x] = hist[t];
}

// Stable scatter: items keep tile order (round-major, lane order inside a
// wave); ranks among equal digits come from per-wave match masks (8 ballots)
// and per-round wave offsets in LDS.
__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(TraceSortArgs a) {
  if (gated(a.gate)) return;
  __shared__ uint32_t goff[256], run[256];
  __shared__ uint32_t wcnt[kSortThreads / kWave][256], woff[kSortThreads / kWave][256];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  goff[t] = a.hist[(uint64_t)t * a.n_tiles + blockIdx.x];
  run[t] = 0;
  for (int k = 0; k < kSortThreads / kWave; k++) wcnt[k][t] = 0;
  __syncthreads();
  const uint32_t* keys = a.keys_in ? a.keys_in : a.key;
  const uint64_t b = (uint64_t)blockIdx.x * kSortTile;
  for (int r = 0; r < kSortRounds; r++) {
    const uint64_t j = b + (uint64_t)r * kSortThreads + t;
    const bool valid = j < a.n_spans;
    const uint32_t k = valid ? keys[j] : 0;
    const uint32_t v = valid ? (a.vals_in ? a.vals_in[j] : (uint32_t)j) : 0;
    const uint32_t d = (k >> a.shift) & 255u;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; bit++) {
      const uint64_t bal = __ballot((d >> bit) & 1u);
      peers &= ((d >> bit) & 1u) ? bal : ~bal;
    }
    const uint32_t rank = __popcll(peers & lanemask_lt(lane));
    const uint32_t cnt = __popcll(peers);
    if (valid && rank == cnt - 1) wcnt[wv][d] = cnt;
    __syncthreads();
    {
      uint32_t acc = run[t];
      for (int k2 = 0; k2 < kSortThreads / kWave; k2++) {
        woff[k2][t] = acc;
        acc += wcnt[k2][t];
        wcnt[k2][t] = 0;
      }
      run[t] = acc;
    }
    __syncthreads();
    if (valid) {
      const uint32_t pos = goff[d] + woff[wv][d] + rank;
      a.keys_out[pos] = k;
      a.vals_out[pos] = v;
    }
  }
}

// ---- exclusive scan of u32 counts --------------------------------------------
__global__ __launch_bounds__(kScanTileItems) void scan_u32_kernel(ScanArgs a) {
  if (gated(a.gate)) return;
  __shared__ uint64_t wsum[kScanTileItems / kWave];
  __shared__ uint64_t prefix;
  __shared__ uint32_t tile_s;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) tile_s = atomicAdd(a.counter, 1u);
  __syncthreads();
  const uint32_t tile = tile_s;
  const uint64_t k = (uint64_t)tile * kScanTileItems + t;
  uint64_t v = 0;
  if (k < a.n)
    v = a.popcount ? (uint64_t)__popcll(static_cast<const uint64_t*>(a.in)[k]) : static_cast<const uint32_t*>(a.in)[k];
  uint64_t incl = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint64_t x = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += x;
  }
  if (lane == kWave - 1) wsum[wv] = incl;
  __syncthreads();
  uint64_t wbase = 0, total = 0;
#pragma unroll
  for (int q = 0; q < kScanTileItems / kWave; q++) {
    const uint64_t x = wsum[q];
    if (q < wv) wbase += x;
    total += x;
  }
  if (wv == 0) {
    const uint64_t pfx = lookback_prefix(a.status, tile, total, a.error);
    if (lane == 0) {
      prefix = pfx;
      if (tile == a.n_tiles - 1 && a.total) *a.total = (uint32_t)(pfx + total);
    }
  }
  __syncthreads();
  if (k < a.n) a.out[k] = (uint32_t)(prefix + wbase + incl - v);
}

// ---- dense per-trace outputs ---------------------------------------------------
__global__ __launch_bounds__(kTThreads) void trace_compact_kernel(TraceCompactArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t w = blockIdx.x * kTWaves + (threadIdx.x >> 6);
  if (w >= a.n_windows) return;
  const uint64_t heads = a.win_heads[w];
  if (!((heads >> lane) & 1)) return;
  const uint32_t t = a.win_base[w] + __popcll(heads & lanemask_lt(lane));
  const TraceRec r = a.rec[(uint64_t)w * kWave + lane];
  if (a.trace_first_span) a.trace_first_span[t] = r.first_span;
  if (a.trace_keep) a.trace_keep[t] = r.keep;
  if (a.trace_level) a.trace_level[t] = r.level;
  if (a.trace_ratio) a.trace_ratio[t] = r.ratio;
}

}  // namespace

void launch_trace_insert_exact(const TraceKernelArgs& a, hipStream_t st) {
  if (a.n_spans)
    hipLaunchKernelGGL(trace_insert_exact_kernel, dim3((uint32_t)std::min<uint64_t>((a.n_spans + 255) / 256, kGatedBlocks)),
                       dim3(256), 0, st, a);
}
void launch_trace_runs(const TraceKernelArgs& a, hipStream_t st) {
  const uint64_t blocks = std::min<uint64_t>((a.n_windows + 3) / 4, kGatedBlocks);
  hipLaunchKernelGGL(trace_runs_kernel, dim3((uint32_t)std::max<uint64_t>(blocks, 1)), dim3(256), 0, st, a);
}
void launch_trace_fold(const TraceKernelArgs& a, hipStream_t st) {
  const uint64_t blocks = std::min<uint64_t>((a.n_windows + kTWaves - 1) / kTWaves, kGatedBlocks);
  hipLaunchKernelGGL(trace_fold_kernel, dim3((uint32_t)std::max<uint64_t>(blocks, 1)), dim3(kTThreads), 0, st, a);
}
void launch_trace_first_select(const TraceKernelArgs& a, hipStream_t st) {
  const uint64_t blocks = std::min<uint64_t>((a.n_windows + 255) / 256, kGatedBlocks);
  hipLaunchKernelGGL(trace_first_select_kernel, dim3((uint32_t)std::max<uint64_t>(blocks, 1)), dim3(256), 0, st, a);
}
void launch_trace_key(const TraceSortArgs& a, hipStream_t st) {
  const uint64_t blocks = std::min<uint64_t>((a.n_spans + 255) / 256, kGatedBlocks);
  hipLaunchKernelGGL(trace_key_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, a);
}
void launch_sort_hist(const TraceSortArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(sort_hist_kernel, dim3(a.n_tiles), dim3(kSortThreads), 0, st, a);
}
void launch_sort_scatter(const TraceSortArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(sort_scatter_kernel, dim3(a.n_tiles), dim3(kSortThreads), 0, st, a);
}
void launch_scan_u32(const ScanArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(scan_u32_kernel, dim3(a.n_tiles), dim3(kScanTileItems), 0, st, a);
}
void launch_trace_compact(const TraceCompactArgs& a, hipStream_t st) {
  const uint32_t blocks = (a.n_windows + kTWaves - 1) / kTWaves;
  hipLaunchKernelGGL(trace_compact_kernel, dim3(blocks), dim3(kTThreads), 0, st, a);
}

}  // namespace ose
