// trace_kernel.hip — the fast path of odigossampling on CDNA4 (gfx950):
// trace_eval_kernel, trace_multi_kernel, the trace_long_* kernels,
// trace_dup_check_kernel, endpoint_plane_kernel and svc_translate_kernel.
// The slow paths: trace_slow_kernel.hip; the trace-id exchange:
// shard_kernel.hip; the device helpers all three share: trace_device.hpp.
//
// Replaces RuleEngine.ShouldSample over every trace of a batch
// (odigossamplingprocessor/rule_engine.go:55-115 with the Evaluate functions
// of internal/sampling/{error,latency,servicename}.go), grouped by trace_id
// as groupbytrace would release them (sampling_controller.go:193-220).
//
// Fast path (one launch): positions are batch order.  A run is a maximal
// stretch of consecutive spans with one trace_id; when every trace_id forms
// exactly one run (groupbytrace release order) each run is a trace.  One
// wave owns the runs whose head lies in its 64-span window and walks them in
// 64-span steps: per-span contributions (error bit, endpoint-match bits of
// the latency rules of the span's service, service-rule bits) are combined
// by wave-segmented scans (DPP, no LDS), the latency state (min start with
// the Go sentinel quirk, max end) by a segmented scan of the latency monoid
// (trace_device.hpp) over stretches of one trace and one latency service.  A
// run that continues past the step is carried in wave-uniform registers plus
// one lane per latency service; a run still open long_steps steps past its
// owner's windows is listed and decided by the trace_long_* kernels.
//
// Duplicate detection: every run head appends a 64-bit fingerprint of its
// trace_id to the bucket its top bits name (flush_heads); per bucket,
// trace_dup_check_kernel puts the fingerprints into an LDS hash set, and one
// met twice, or a bucket past kDupBucketCap, sets *dup.  Different ids with
// one fingerprint only send the batch to the slow paths, which compare ids.
//
// Gating: the fast pass runs in every SAMPLE call; the sorted (kTracePerm)
// pass of trace_eval_kernel returns at once unless its *dup word is set; the
// trace_long_* kernels read the listed-run and piece counts (n_long) from
// device memory, and workgroups past them exit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "trace_device.hpp"

namespace ose {
namespace {

// A latency slot with two or more stretches in one closed trace (rep: a
// stretch head whose slot the trace already had): the OR of its stretches'
// results (lsat = lraw & ep, set by the caller) is not the trace's, so that
// slot's monoid is scanned over the whole trace and its rules' bits replaced
// at the trace's tail.  Only the repeated slots are rescanned (a step with
// one repeat used to rescan every slot of its closed traces).
__device__ __forceinline__ void rep_slots(const Cfg& c, bool rep, uint32_t slot, uint32_t hseg, bool ttail, uint64_t st,
                                       uint64_t en, uint32_t rst, uint64_t ep, uint64_t& lsat) {
  // the trace's repeated slots (a segmented OR of the rep lanes' slot bits)
  uint32_t rlo = rep && slot < 32 ? 1u << slot : 0u, rhi = rep && slot >= 32 && slot != kNoSlot ? 1u << (slot - 32) : 0u;
  seg_or_scan(hseg, rlo, rhi);
  const uint64_t rm = (uint64_t)rlo | ((uint64_t)rhi << 32);
  for (uint64_t pend = __ballot(rep); pend;) {
    const uint32_t ks = lane_value(slot, ffs64(pend));
    const bool ink = slot == ks;
    pend &= ~__ballot(ink);
    Lat v = ink ? LAT_OF_SPAN(st, en, rst) : Lat{0u, kInf, 0ull};
    seg_lat_scan(hseg, v);
    if (ttail && ((rm >> ks) & 1))
      lsat = (lsat & ~c.slot_rules[ks]) | ((v.f & 2u) ? latency_satisfied(c, ks, ep, v.m, v.e) : 0ull);
  }
}

// load_cfg() with the table offsets in scalar registers: read from LDS they
// arrive in vector registers although every lane reads the same header, and
// the six table addresses then hold six VGPRs for the whole kernel
__device__ __forceinline__ Cfg load_cfg_uniform(const uint8_t* b) {
  Cfg c;
  c.h = reinterpret_cast<const SampCfgDev*>(b);
  c.rules = reinterpret_cast<const SampRuleDev*>(b + sgpr(c.h->rules_off));
  c.lat = reinterpret_cast<const SampLatDev*>(b + sgpr(c.h->lat_off));
  c.svc_slot = reinterpret_cast<const uint32_t*>(b + sgpr(c.h->svc_slot_off));
  c.slot_rules = reinterpret_cast<const uint64_t*>(b + sgpr(c.h->slot_rules_off));
  c.svc_bits = reinterpret_cast<const uint64_t*>(b + sgpr(c.h->svc_bits_off));
  c.bytes = b + sgpr(c.h->bytes_off);
  return c;
}

// ---- per-step columns ---------------------------------------------------------
// Raw loads of one 64-span step, issued one step ahead of their use and first
// waited for at the top of the next iteration, so a wave's column reads of
// step s+1 are in flight while step s is computed.  vmcnt counts loads in
// order and the compiler can only count what it can see, so three rules keep
// a later wait from draining the prefetch (profiles/trace_prefetch_isa.txt):
//  - values stay as loaded (status is the byte; no conversion or select in
//    the block that loads);
//  - no load sits under a divergent branch: the span index is clamped to
//    n - 1 (a lane past the batch's end reads the last span's columns, which
//    nothing uses: every use is under valid / mine), and the neighbour trace
//    id is one load whose address is selected per lane; only wave-uniform
//    decisions (full, a column that is not configured) branch;
//  - the step's dependent loads (service ids, route window, route_match) are
//    consumed before the prefetch is issued (trace_eval_kernel).
struct StepRaw {
  uint64_t i;          // span index (perm[p] in kTracePerm)
  uint64_t hi, lo;     // trace id
  uint64_t ph, pl;     // lane 0: trace id of position p-1 (head test); lane 63: of p+1 (kTraceRuns)
  uint32_t k, pk;      // kTracePerm: canonical key of p and (lane 0) of p-1
  uint32_t res;
  uint8_t status;      // as loaded; widened where it is used
  ose_strref route;
  uint64_t start, end;
  uint64_t svm;        // svc_match (owner-side record columns)
  bool full;           // the per-span columns below the trace id were loaded
};
// a value's load has to have arrived here: the wait for it (and, vmcnt being
// in order, for every load issued before it) is placed at this point
__device__ __forceinline__ void consume(uint32_t x) { asm volatile("" ::"v"(x)); }
// Comments in the machine code that tools/vmcnt_report.py reads: the end of
// the prefetch, and the blocks that run once per many steps and wait for a
// returning atomic or end in stores (the queue flushes, the long-run
// hand-off).  No instructions.
#define OSE_MARK(what) asm volatile("; ose." what)
// full = false loads only what the head test needs: a wave skipping windows
// inside a run an earlier wave owns reads 16 B per span, not every column.
// n_spans > 0 (the callers').
// res = false leaves the resource index out (trace_eval_kernel's lean
// instances load it two steps ahead).
__device__ __forceinline__ StepRaw load_raw(const TraceKernelArgs& a, uint64_t base, int lane, bool full = true,
                                            bool res = true) {
  StepRaw r{};
  r.full = full;
  const uint64_t last = a.n_spans - 1;
  const uint64_t p = min(base + lane, last);
  if (a.mode == kTracePerm) {
    r.i = a.perm[p];
    r.k = a.key[r.i];
    r.pk = a.key[a.perm[p > 0 ? p - 1 : 0]];   // (lane 0's is used)
  } else {
    r.i = p;
    if (a.mode == kTraceRuns) {
      // lane 0: the span before the step; lane 63: the span after it; the
      // other lanes read their own id again (the same cache lines)
      const uint64_t q = lane == 0 ? (p > 0 ? p - 1 : 0) : (lane == kWave - 1 ? min(p + 1, last) : p);
      const uint4 w = reinterpret_cast<const uint4*>(a.tid)[q];
      r.ph = (uint64_t)w.x | ((uint64_t)w.y << 32);
      r.pl = (uint64_t)w.z | ((uint64_t)w.w << 32);
    }
  }
  const uint4 v = reinterpret_cast<const uint4*>(a.tid)[r.i];
  r.hi = (uint64_t)v.x | ((uint64_t)v.y << 32);
  r.lo = (uint64_t)v.z | ((uint64_t)v.w << 32);
  if (!full) return r;
  if (res) r.res = a.resource[r.i];
  r.status = a.status[r.i];
  if (a.start) {
    r.start = a.start[r.i];
    r.end = a.end[r.i];
  }
  if (a.route) r.route = a.route[r.i];
  if (a.svc_match) r.svm = a.svc_match[r.i];
  return r;
}
// The columns of a step whose prefetch was a skip-mode one, loaded at its top
// and waited for there, all of them (vmcnt(0), the other counters left alone):
// once per wave, and no later wait then has a load of this step to wait for.
__device__ __forceinline__ StepRaw reload_raw(const TraceKernelArgs& a, uint64_t base, int lane) {
  const StepRaw r = load_raw(a, base, lane);
  __builtin_amdgcn_s_waitcnt(0x0F70);
  return r;
}
// head flag of every lane of a step (all lanes take the shuffles)
__device__ __forceinline__ bool step_head(const TraceKernelArgs& a, const StepRaw& r, uint64_t base, int lane) {
  const uint64_t p = base + lane;
  const bool valid = p < a.n_spans;
  if (a.mode == kTracePerm) {
    uint32_t pk = __shfl_up(r.k, 1, kWave);
    if (lane == 0) pk = r.pk;
    return valid && (p == 0 || pk != r.k);
  }
  // wave_shr:1 (DPP): lane l gets lane l-1's trace id, lane 0 its own prefetched p-1 id
  const uint64_t ph = dpp_mov64<0x138, 0xF>(r.ph, r.hi), pl = dpp_mov64<0x138, 0xF>(r.pl, r.lo);
  if (a.mode == kTraceBatch) return valid && p == 0;
  return valid && (p == 0 || ph != r.hi || pl != r.lo);
}
__device__ __forceinline__ bool head_at(const TraceKernelArgs& a, uint64_t p) {   // p < n, p > 0
  if (a.mode == kTraceBatch) return false;
  if (a.mode == kTracePerm) return a.key[a.perm[p]] != a.key[a.perm[p - 1]];
  return a.tid[2 * p] != a.tid[2 * p - 2] || a.tid[2 * p + 1] != a.tid[2 * p - 1];
}

// Run heads are collected per wave in LDS and inserted 64 at a time: each
// insert is a load and a dependent CAS, so batching turns a per-step pair of
// round trips into one pair per 64 heads.
constexpr int kHeadQ = 128;
struct HeadQ {
  uint64_t cell[kHeadQ];
};
// a run head's cell: one multiply (odd: a bijection) on the folded id; its
// top bits (the bucket) depend on every bit of the id
__device__ __forceinline__ uint64_t head_fingerprint(uint64_t hi, uint64_t lo) {
  return (lo ^ ((hi << 29) | (hi >> 35))) * 0x9E3779B97F4A7C15ull;
}
__device__ void flush_heads(const TraceKernelArgs& a, HeadQ& H, uint32_t& hn, int lane) {
  __builtin_amdgcn_wave_barrier();
  OSE_MARK("flush begin");
  bool dup = false;
  // bucketed: one returning atomic per head, the fingerprint stored after it
  for (uint32_t b = 0; b < hn; b += kWave) {
    if (b + lane < hn) {
      const uint64_t h = H.cell[b + lane];
      const uint32_t bk = (uint32_t)(h >> (64 - a.dup_bkt_bits));   // dup_bkt_bits in [1, 32] (the host's)
      const uint32_t at = atomicAdd(&a.dup_bkt_count[bk], 1u);
      if (at < kDupBucketCap) a.dup_bkt[(uint64_t)bk * kDupBucketCap + at] = h | 1ull;   // (0 marks an empty set slot)
      else dup = true;
    }
  }
  // one *dup store per wave flush (a per-head atomic on one word serialises)
  if (__ballot(dup) && lane == 0) atomicOr(a.dup, 1u);
  OSE_MARK("flush end");
  __builtin_amdgcn_wave_barrier();
  hn = 0;
}
// the run heads of a step (hmask != 0; hd: this lane is one) into the wave's queue
__device__ __forceinline__ void queue_heads(const TraceKernelArgs& a, HeadQ& H, uint32_t& hn, uint64_t hmask, bool hd,
                                            uint64_t hi, uint64_t lo, int lane) {
  const uint32_t nh = __popcll(hmask);
  if (hn + nh > kHeadQ) flush_heads(a, H, hn, lane);
  if (hd) {
    const uint32_t e = hn + __popcll(hmask & lanemask_lt(lane));
    H.cell[e] = head_fingerprint(hi, lo);
  }
  hn += nh;
}

// ---- decide queue ---------------------------------------------------------------
// Closed traces are queued per wave in LDS and decided 64 at a time, so the
// rule fold runs with every lane busy instead of once per trace tail.
constexpr int kQ = 64;
struct DecideQ {
  uint64_t ep[kQ], lsat[kQ], svc[kQ], hi[kQ], lo[kQ];
  uint32_t pos[kQ], len[kQ], err[kQ];
};

__device__ __forceinline__ void write_keep_range(const TraceKernelArgs& a, uint64_t pos, uint32_t len, uint8_t k,
                                                 int lane) {
  for (uint32_t q = lane; q < len; q += kWave) a.keep[a.mode == kTracePerm ? a.perm[pos + q] : pos + q] = k;
}

__device__ void flush_queue(const TraceKernelArgs& a, const Cfg& c, DecideQ& Q, uint32_t& qn, int lane) {
  if (!qn) return;
  __builtin_amdgcn_wave_barrier();
  OSE_MARK("flush begin");
  uint8_t dk = 0, dl = 0;
  double dr = 0;
  uint32_t pos = 0, len = 0;
  if ((uint32_t)lane < qn) {
    pos = Q.pos[lane];
    len = Q.len[lane];
    if (!(a.ablate & 4))
      decide_at(a, c, a.mode == kTracePerm ? a.perm[pos] : (a.mode == kTraceBatch ? 0u : pos), Q.err[lane], Q.ep[lane],
                Q.lsat[lane], Q.svc[lane], trace_uniform(Q.hi[lane], Q.lo[lane], a.seed), dk, dl, dr);
    write_rec(a, pos, dk, dl, dr);
  }
  const uint32_t mlen = wave_max_u32((uint32_t)lane < qn ? len : 0u);
  if (a.mode != kTracePerm && mlen <= 32) {
    // short traces: each lane writes its own trace's keep bytes (at most 32
    // store instructions per 64 traces instead of one per trace)
    if ((uint32_t)lane < qn)
      for (uint32_t q = 0; q < len; q++) a.keep[pos + q] = dk;
  } else {
    for (uint32_t e = 0; e < qn; e++)
      write_keep_range(a, lane_value(pos, e), lane_value(len, e), (uint8_t)lane_value(dk, e), lane);
  }
  OSE_MARK("flush end");
  __builtin_amdgcn_wave_barrier();
  qn = 0;
}

// kLean: the instance for the common call — batch order (kTraceRuns), no
// owner-side record columns, no precomputed endpoint bits, no span_attribute
// bits, no diagnostics.  Those arguments are constants in it, so their code
// and the kernel-argument registers that hold them fold away (the general
// instance spills ~90 scalar registers into vector lanes).
// kNarrow (with kLean): the error bit, the endpoint bits of the latency rules
// and the service-rule bits fit one 32-bit word (1 + n_lat + service bits <=
// 32, n_lat_slots <= 32; the host checks): the segmented ORs scan one word
// instead of five, the latency stretches' words two instead of four.
// kChunk (with kLean): one pass of a rule-chunked configuration, the walk
// resumed from fold_in and saved to fold_out (decide_chunk) — the lean
// instance's loads and scans instead of the general instance's.
template <bool kLean, bool kNarrow, bool kChunk>
__global__ __launch_bounds__(kTThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void trace_eval_kernel(TraceKernelArgs a) {
  if (kLean) {
    a.mode = kTraceRuns;
    a.svc_match = nullptr;
    a.route_match = nullptr;
    a.attr_match = nullptr;
    a.perm = nullptr;
    a.key = nullptr;
    a.batch_keep = nullptr;
#if !OSE_DIAG
    a.ablate = 0;   // (diagnostics builds keep OSE_TRACE_ABLATE for the lean instances too)
#endif
    if (!kChunk) {
      a.fold_in = nullptr;
      a.fold_out = nullptr;
    }
  }
  if (a.mode == kTracePerm && __hip_atomic_load(a.dup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  __shared__ DecideQ queues[kTWaves];
  __shared__ HeadQ headqs[kTWaves];
  __shared__ __attribute__((aligned(16))) uint8_t cfg_lds[kSampCfgLds];
  const int lane = threadIdx.x & 63;
  const uint32_t wv = threadIdx.x >> 6;
  DecideQ& Q = queues[wv];
  HeadQ& HQ = headqs[wv];
  // the rule tables (<= kSampCfgLds bytes, checked by the host) live in LDS:
  // every lookup below is a ds_read instead of a dependent L2 round trip
  copy_cfg_to_lds<kTThreads>(cfg_lds, a.cfg);
  __syncthreads();
  const uint64_t wpw = a.win_per_wave;
  const uint64_t w0 = ((uint64_t)blockIdx.x * kTWaves + wv) * wpw;   // first owned window
  if (w0 >= a.n_windows) return;
  const Cfg c = load_cfg_uniform(cfg_lds);
  const uint64_t n = a.n_spans;
  const uint32_t nsvc = c.h->n_services;

  // OSE_GROUP_BATCH: ServiceNameRule looks at every resource of the call,
  // spanless ones included (servicename.go:38-47).
  uint64_t batch_svc = 0;
  if (a.mode == kTraceBatch && w0 == 0) {
    for (uint32_t r = lane; r < a.n_resources; r += kWave) {
      const uint32_t s = a.res_svc_str[r];
      if (s < nsvc) batch_svc |= c.svc_bits[s];
    }
    batch_svc = wave_or64(batch_svc);
  }
  if (n == 0) {   // kTraceBatch only: one trace with no spans
    uint8_t k, l;
    double r;
    decide_at(a, c, 0, 0, 0, 0, batch_svc, trace_uniform(0, 0, a.seed), k, l, r);
    if (lane == 0) {
      if (a.batch_keep) *a.batch_keep = k;
      if (a.win_heads) a.win_heads[0] = 1;
      if (a.rec) {
        TraceRec rr{0, k, l, 0, 0, r};
        a.rec[0] = rr;
      }
    }
    return;
  }

  const uint64_t range_end = min((w0 + wpw) * kWave, n);
  uint32_t qn = 0, hn = 0;
  bool started = false, open = false;
  uint32_t c_err = 0;
  uint64_t c_ep = 0, c_svc = 0, c_kmask = 0, c_pos = 0, c_hi = 0, c_lo = 0;
  Lat cur{0, kInf, 0};
  uint64_t base = w0 * kWave;
  const bool want_route = c.h->n_lat && !a.route_match && a.route;
  // kPipe (the lean instances: batch order, span index = position): the
  // dependent chain runs a step ahead of the columns' use.  The resource index
  // is loaded two steps ahead, the service ids of step s+1 are issued in step
  // s, in front of its prefetch, and arrive with it: a step waits for the
  // route window alone.  The pipelined values exist only while the wave
  // evaluates (a skipped step loads trace ids and nothing else); the first
  // evaluated step loads its own (prime) and waits.
  constexpr bool kPipe = kLean;
  uint32_t p_sv = 0, p_ss = 0, p_res = 0;   // kPipe: service ids of this step, resource index of the next
  // the columns of the step at b in full, its service ids, the next step's resource index
  auto prime = [&](uint64_t b) {
    const StepRaw x = load_raw(a, b, lane);
    if constexpr (kPipe) {
      p_res = a.resource[min(b + kWave + lane, n - 1)];
      p_sv = a.res_svc[x.res];
      p_ss = a.res_svc_str[x.res];
    }
    return x;
  };
  StepRaw nx = prime(base);
  for (;;) {
    // Order of the memory operations per step: this step's dependent loads
    // (resource service ids unless kPipe, the route window, the fingerprint
    // cell), then the next step's service ids (kPipe) and column loads, then
    // the arithmetic — a wait for a load also waits for every load issued
    // before it (vmcnt counts in order), so nothing this step consumes may be
    // issued after the prefetch.
    StepRaw r = nx;
    const bool valid = base + lane < n;
    const bool hd = step_head(a, r, base, lane);
    const bool work = started || __ballot(hd) != 0;   // wave-uniform: this step is evaluated
    if (work && !r.full) {   // first owned step after skipped ones: everything of it, waited for (vmcnt(0))
      r = prime(base);
      __builtin_amdgcn_s_waitcnt(0x0F70);
    }
    // Everything that reads memory through this step's columns is finished
    // here, before the prefetch: the service ids, the latency slot, and the
    // endpoint bits (route window, the bytes of a prefix past it, route_match).
    uint32_t ss = 0xFFFFFFFFu, slot0 = kNoSlot;
    uint64_t ep0 = 0;
    if (valid && work) {
      uint32_t sv;
      if constexpr (kPipe) {
        sv = p_sv;
        ss = p_ss;
      } else if (a.ablate & 16) {   // diagnostics: no dependent service-id loads
        sv = r.res % (nsvc + 1);
        ss = sv;
      } else {
        sv = a.res_svc[r.res];
        ss = a.res_svc_str[r.res];
        consume(ss);   // (not used before the prefetch otherwise)
      }
      if (sv < nsvc) {
        slot0 = c.svc_slot[sv];
        if (slot0 != kNoSlot && !(a.ablate & 8)) {
          if (a.route_match) {
            ep0 = a.route_match[r.i] & c.slot_rules[slot0];
          } else {
            // route bytes only for spans of a latency-rule service (strings.HasPrefix
            // is evaluated for nothing else): one dependent LDS lookup, and the
            // random 16-byte arena reads of every other routed span are skipped
            uint4 rw = make_uint4(0, 0, 0, 0);
            if (want_route && r.route.len && !(a.ablate & 32)) rw = head16(a.arena, r.route.off, r.route.len);
            ep0 = endpoint_bits_w(c, slot0, a.arena, r.route, rw);
          }
        }
      }
    }
    // kPipe: the youngest load of the last prefetch, so every column of this step is here
    if constexpr (kPipe) consume(p_res);
    const uint64_t vmask = __ballot(valid);
    const uint64_t hmask = __ballot(hd);
    const bool in_range = base < range_end;
    if (in_range) {
      if (lane == 0 && a.win_heads) a.win_heads[base / kWave] = hmask;
      // (no dup_bkt: a later rule-chunk pass, whose batch layout the first
      // pass already checked — *dup carries that pass's answer)
      if (a.mode == kTraceRuns && !(a.ablate & 1) && a.dup_bkt && hmask)
        queue_heads(a, HQ, hn, hmask, hd, r.hi, r.lo, lane);
    }
    if (base + kWave < n) {   // prefetch the next step
      if constexpr (kPipe) {
        if (work) {   // (with a.ablate & 16, diagnostics: no dependent service-id loads)
          p_sv = (a.ablate & 16) ? p_res % (nsvc + 1) : a.res_svc[p_res];
          p_ss = (a.ablate & 16) ? p_sv : a.res_svc_str[p_res];
        }
      }
      nx = load_raw(a, base + kWave, lane, work, !kPipe);
      if constexpr (kPipe) {
        if (work) p_res = a.resource[min(base + 2 * kWave + lane, n - 1)];
      }
    }
    OSE_MARK("prefetch issued");
    uint64_t own;
    if (in_range) {
      if (!started) {
        if (!hmask) {   // still inside a trace an earlier wave owns
          base += kWave;
          if (base >= range_end) break;
          continue;
        }
        started = true;
        own = vmask & ~lanemask_lt(ffs64(hmask));
      } else {
        own = vmask;
      }
    } else {
      if (!open) break;
      own = vmask & (hmask ? lanemask_lt(ffs64(hmask)) : ~0ull);
    }
    const uint64_t segmask = (hmask & own) | (open ? 1ull : 0ull);
    const int last_own = fls64(own);
    bool cont_next = false;
    if (last_own == 63 && base + kWave < n) {
      bool h = false;
      // kTraceRuns: lane 63 loaded the next step's first trace id with this step
      if (lane == 63) h = a.mode == kTraceRuns ? (r.ph != r.hi || r.pl != r.lo) : head_at(a, base + kWave);
      cont_next = !lane_value((uint32_t)h, 63);
    }
    const bool mine = (own >> lane) & 1;
    const int sst = mine ? fls64(segmask & lanemask_le(lane)) : lane;
    const bool tail = mine && (lane == last_own || ((segmask >> (lane + 1)) & 1));
    const uint64_t tails = __ballot(tail);
    const int t0 = ffs64(tails);
    const bool seg0_cont = open;
    const bool single = t0 == last_own;
    const bool last_open = cont_next && !(single && seg0_cont);   // a new trace opens in this step and continues
    const int sst_last = lane_value((uint32_t)sst, last_own);

    // ---- per-span contributions ----
    uint32_t err = 0, slot = kNoSlot;
    uint64_t ep = 0, svcb = 0, st = 0, en = 0;
    const uint32_t rst = (r.status & kStatusReset) ? 1u : 0u;   // owner-side record: a zero start came first
    if (mine) {
      err = ((uint32_t)r.status & ~kStatusReset) == OSE_STATUS_ERROR;
      if (a.svc_match) {
        svcb = r.svm;
      } else {
        if (a.mode != kTraceBatch && ss < nsvc) svcb = c.svc_bits[ss];
        if (a.attr_match) svcb |= chunk_attr_bits(a.attr_match, a.attr_stride, a.attr_words, c.h, r.i);
      }
      slot = slot0;
      if (slot != kNoSlot) {
        ep = ep0;
        st = r.start;
        en = r.end;
      }
    }
    // ---- latency state (latency.go:69-80) ----
    // One segmented scan of the monoid over stretches: maximal runs of lanes
    // with one trace and one latency slot (a trace's spans of a service come
    // together, ResourceSpans by ResourceSpans).  A stretch's element is its
    // trace's element for that slot when the slot has no other stretch in the
    // trace within this step; the step checks that (slot bits OR-scanned per
    // trace) and otherwise takes the per-slot scans below.  At a stretch tail
    // the slot's rules whose threshold the duration reaches are found without
    // the endpoint mask; ORed per trace and masked by the trace's endpoint bits
    // at its tail, they are the per-slot result.  The carried trace (segment 0)
    // and the trace left open at the end combine their stretches into the
    // per-slot carry registers in lane order.
    const uint32_t hseg = mine ? (uint32_t)((segmask >> lane) & 1) : 1u;
    // ---- segmented OR of the flag masks (DPP scan; h = segment head) ----
    if constexpr (kNarrow) {
      const uint32_t nsh = 1 + c.h->n_lat;   // <= 32 (host-checked)
      uint32_t pk = err | ((uint32_t)ep << 1) | (nsh < 32 ? (uint32_t)svcb << nsh : 0u);
      seg_or_scan(hseg, pk);
      err = pk & 1u;
      ep = (pk >> 1) & (uint32_t)((1ull << c.h->n_lat) - 1);
      svcb = nsh < 32 ? pk >> nsh : 0u;
    } else {
      seg_or_scan(hseg, err, ep, svcb);
    }
    uint64_t lsat = 0, n_kmask = 0;
    Lat nxt{0, kInf, 0};
    const bool carried_tail = (lane == t0 && seg0_cont) || (lane == last_own && last_open);
    const bool lat_on = !(a.ablate & 2) && __ballot(slot != kNoSlot) != 0;   // wave-uniform
    uint64_t lraw = 0, smask = 0;
    bool stail = false, shead = false;
    if (lat_on) {
      const uint32_t pslot = dpp_mov<0x138>(kNoSlot, slot);   // lane - 1's slot (wave_shr:1)
      shead = !mine || hseg || pslot != slot;
      const uint32_t hs = shead ? 1u : 0u;
      stail = mine && dpp_mov<0x130>(1u, hs) != 0;            // lane + 1 starts a stretch (wave_shl:1)
      Lat v = slot != kNoSlot ? LAT_OF_SPAN(st, en, rst) : Lat{0u, kInf, 0ull};
      seg_lat_scan(hs, v);
      const bool lt = stail && (v.f & 2u);
      if (lt) lraw = latency_satisfied(c, slot, ~0ull, v.m, v.e);
      if (slot != kNoSlot) smask = 1ull << slot;
      if (seg0_cont) {   // the carried trace's stretches, in order
        for (uint64_t m0 = __ballot(lt && lane <= t0); m0; m0 &= m0 - 1) {
          const int L = ffs64(m0);
          const uint32_t ks = lane_value(slot, L);
          const Lat v0{lane_value(v.f, L), lane_value64(v.m, L), lane_value64(v.e, L)};
          if ((uint32_t)lane == ks) cur = lat_comb(cur, v0);
          c_kmask |= 1ull << ks;
        }
      }
      if (last_open) {   // the open trace's stretches, in order
        for (uint64_t m1 = __ballot(lt && lane >= sst_last); m1; m1 &= m1 - 1) {
          const int L = ffs64(m1);
          const uint32_t ks = lane_value(slot, L);
          const Lat v1{lane_value(v.f, L), lane_value64(v.m, L), lane_value64(v.e, L)};
          if ((uint32_t)lane == ks) nxt = lat_comb(nxt, v1);
          n_kmask |= 1ull << ks;
        }
      }
    }
    if (lat_on) {
      if constexpr (kNarrow) {
        uint32_t lr = (uint32_t)lraw, sm = (uint32_t)smask;
        seg_or_scan(hseg, lr, sm);
        lraw = lr;
        smask = sm;
      } else {
        seg_or_scan(hseg, lraw, smask);
      }
      // a slot with two stretches in a trace this step closes: per-slot scans
      const uint64_t psm = dpp_mov64<0x138, 0xF>(0ull, smask);   // lane - 1's inclusive slot bits
      const bool in_closed = mine && !(seg0_cont && lane <= t0) && !(last_open && lane >= sst_last);
      const bool rep = in_closed && shead && !hseg && slot != kNoSlot && ((psm >> slot) & 1);
      if (tail && !carried_tail) lsat = lraw & ep;
      if (__ballot(rep)) rep_slots(c, rep, slot, hseg, tail && !carried_tail, st, en, rst, ep, lsat);
    }
    // ---- the carried trace closes in this step: queue it ----
    const bool cont_close = seg0_cont && !(single && cont_next);
    if (cont_close) {
      const uint32_t E = c_err | lane_value(err, t0);
      const uint64_t EP = c_ep | lane_value64(ep, t0);
      const uint64_t SV = batch_svc | c_svc | lane_value64(svcb, t0);
      uint64_t s_l = 0;
      if ((c_kmask >> lane) & 1) s_l = latency_satisfied(c, (uint32_t)lane, EP, cur.m, cur.e);
      s_l = wave_or64(s_l);
      if (qn == kQ) flush_queue(a, c, Q, qn, lane);
      if (lane == 0) {
        Q.err[qn] = E;
        Q.ep[qn] = EP;
        Q.lsat[qn] = s_l;
        Q.svc[qn] = SV;
        Q.hi[qn] = c_hi;
        Q.lo[qn] = c_lo;
        Q.pos[qn] = (uint32_t)c_pos;
        Q.len[qn] = (uint32_t)(base + t0 + 1 - c_pos);
      }
      qn++;
      open = false;
      cur = Lat{0, kInf, 0};
      c_kmask = 0;
    }
    // ---- traces that start and end in this step: queue them ----
    const uint64_t qmask = __ballot(tail && !carried_tail);
    const uint32_t nq = __popcll(qmask);
    if (nq) {
      if (qn + nq > kQ) flush_queue(a, c, Q, qn, lane);
      // the trace's first span's id (the injected uniform): in batch order and
      // in the sorted permutation every span of a segment has that id; only a
      // whole-batch trace (OSE_GROUP_BATCH) mixes ids
      uint64_t hh = r.hi, hl = r.lo;
      if (a.mode == kTraceBatch) {
        hh = __shfl(r.hi, sst, kWave);
        hl = __shfl(r.lo, sst, kWave);
      }
      if ((qmask >> lane) & 1) {
        const uint32_t e = qn + __popcll(qmask & lanemask_lt(lane));
        Q.err[e] = err;
        Q.ep[e] = ep;
        Q.lsat[e] = lsat;
        Q.svc[e] = batch_svc | svcb;   // batch mode: resource bits of the call + span_attribute bits
        Q.hi[e] = hh;
        Q.lo[e] = hl;
        Q.pos[e] = (uint32_t)(base + sst);
        Q.len[e] = (uint32_t)(lane - sst + 1);
      }
      qn += nq;
    }
    // ---- carry into the next step ----
    if (last_open) {
      open = true;
      c_pos = base + sst_last;
      c_hi = lane_value64(r.hi, sst_last);
      c_lo = lane_value64(r.lo, sst_last);
      c_err = lane_value(err, last_own);
      c_ep = lane_value64(ep, last_own);
      c_svc = lane_value64(svcb, last_own);
      cur = nxt;
      c_kmask = n_kmask;
    } else if (seg0_cont && single && cont_next) {
      c_err |= lane_value(err, t0);
      c_ep |= lane_value64(ep, t0);
      c_svc |= lane_value64(svcb, t0);
    }
    base += kWave;
    if (!open && base >= range_end) break;
    if (open && a.long_runs && base >= range_end + (uint64_t)a.long_steps * kWave) {
      // a long run: trace_long_kernel splits it over a workgroup's waves
      OSE_MARK("flush begin");   // (the hand-off: the wave's last step)
      if (lane == 0) a.long_runs[atomicAdd(a.n_long, 1u)] = (uint32_t)c_pos;
      OSE_MARK("flush end");
      break;
    }
  }
  flush_queue(a, c, Q, qn, lane);
  if (a.dup_bkt) flush_heads(a, HQ, hn, lane);
}

// ---- rule-chunked lists in one pass ---------------------------------------------
// A rule list cut into K (2..kMaxMulti) chunks — no span_attribute rules, no
// spilled routes, grouped by trace id — in one pass over the columns instead
// of one per chunk: every chunk's table sits in LDS, each step evaluates each
// chunk's endpoint, service and latency words exactly as trace_eval_kernel
// does for one table, and a closed trace is queued with all K; the flush
// walks the chunks in order (walk_chunk, then walk_finish: decide() over the
// whole list, rule_engine.go:55-115).  Duplicate detection is the lean
// instance's; a batch whose trace ids repeat is redone by the pass-per-chunk
// path (run_sampling).  No long-run hand-off: a run's owner wave follows it.
template <int K>
struct MultiQ {
  uint64_t hi[kQ], lo[kQ];
  uint32_t pos[kQ], len[kQ], err[kQ];
  uint64_t ep[K][kQ], lsat[K][kQ], svc[K][kQ];
};

template <int K>
__device__ __forceinline__ void flush_multi(const TraceKernelArgs& a, const uint8_t* lds, const uint32_t (&coff)[K],
                                            const SampWalkDev* walks, MultiQ<K>& Q, uint32_t& qn, int lane) {
  if (!qn) return;
  __builtin_amdgcn_wave_barrier();
  OSE_MARK("flush begin");
  uint8_t dk = 0, dl = 0;
  double dr = 0;
  uint32_t pos = 0, len = 0;
  if ((uint32_t)lane < qn) {
    pos = Q.pos[lane];
    len = Q.len[lane];
    FoldState s{0.0, 0.0, 0u, 0u};
    const uint32_t err = Q.err[lane];
#pragma unroll
    for (int k = 0; k < K; k++)
      walk_sparse(load_cfg(lds + coff[k]), walks[k], s, err, Q.ep[k][lane], Q.lsat[k][lane], Q.svc[k][lane]);
    walk_finish(s, trace_uniform(Q.hi[lane], Q.lo[lane], a.seed), dk, dl, dr);
    write_rec(a, pos, dk, dl, dr);
  }
  const uint32_t mlen = wave_max_u32((uint32_t)lane < qn ? len : 0u);
  if (mlen <= 32) {
    if ((uint32_t)lane < qn)
      for (uint32_t q = 0; q < len; q++) a.keep[pos + q] = dk;
  } else {
    for (uint32_t e = 0; e < qn; e++) write_keep_range(a, lane_value(pos, e), lane_value(len, e), (uint8_t)lane_value(dk, e), lane);
  }
  OSE_MARK("flush end");
  __builtin_amdgcn_wave_barrier();
  qn = 0;
}

template <int K>
__global__ __launch_bounds__(kTThreads) __attribute__((amdgpu_waves_per_eu(2, 4))) void trace_multi_kernel(TraceKernelArgs a) {
  extern __shared__ uint4 multi_cfg4[];
  uint8_t* mcfg = reinterpret_cast<uint8_t*>(multi_cfg4);
  __shared__ MultiQ<K> queues[kTWaves];
  __shared__ HeadQ headqs[kTWaves];
  const int lane = threadIdx.x & 63;
  const uint32_t wv = threadIdx.x >> 6;
  MultiQ<K>& Q = queues[wv];
  HeadQ& HQ = headqs[wv];
  uint32_t coff[K];
  const uint32_t nsvc = reinterpret_cast<const SampCfgDev*>(a.cfgs[0])->n_services;   // (the engine's: every chunk's)
  const uint32_t* gslot_of;   // LDS: latency-service index of each service, then the service of each index
  const SampWalkDev* wlk;     // LDS: each chunk's rules by what matches them
  {
    // every chunk's table (each <= kSampCfgLds, together <= kMultiCfgLds with
    // the latency-service ids: the host checks) into LDS
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
      // (written out: copy_cfg_to_lds here changes this kernel's code)
      const uint8_t* g = a.cfgs[k];
      const uint32_t nb = cfg_lds_copy_bytes(g);
      for (uint32_t x = threadIdx.x * 16; x < nb; x += kTThreads * 16)
        *reinterpret_cast<uint4*>(mcfg + o + x) = *reinterpret_cast<const uint4*>(g + x);
      coff[k] = o;
      o += (nb + 15u) & ~15u;
    }
    uint32_t* gl = reinterpret_cast<uint32_t*>(mcfg + o);
    for (uint32_t x = threadIdx.x; x < nsvc + 64; x += kTThreads) gl[x] = a.lat_gslot[x];
    gslot_of = gl;
    o += ((nsvc + 64) * 4 + 15u) & ~15u;
    // each chunk's SampWalkDev (16-byte multiples)
    const uint4* wg = reinterpret_cast<const uint4*>(a.walks);
    uint4* wl = reinterpret_cast<uint4*>(mcfg + o);
    for (uint32_t x = threadIdx.x; x < K * sizeof(SampWalkDev) / 16; x += kTThreads) wl[x] = wg[x];
    wlk = reinterpret_cast<const SampWalkDev*>(mcfg + o);
    __syncthreads();
  }
  const uint32_t* gsvc = gslot_of + nsvc;
  const uint64_t wpw = a.win_per_wave;
  const uint64_t w0 = ((uint64_t)blockIdx.x * kTWaves + wv) * wpw;   // first owned window
  if (w0 >= a.n_windows) return;
  const uint64_t n = a.n_spans;

  const uint64_t range_end = min((w0 + wpw) * kWave, n);
  uint32_t qn = 0, hn = 0;
  bool started = false, open = false;
  uint32_t c_err = 0;
  uint64_t c_pos = 0, c_hi = 0, c_lo = 0, c_kmask = 0;
  Lat cur{0, kInf, 0};   // lane g: the open trace's latency monoid for latency service g
  uint64_t c_ep[K], c_svc[K];
#pragma unroll
  for (int k = 0; k < K; k++) c_ep[k] = c_svc[k] = 0;
  uint64_t base = w0 * kWave;
  StepRaw nx = load_raw(a, base, lane);
  for (;;) {
    StepRaw r = nx;
    const bool valid = base + lane < n;
    const bool hd = step_head(a, r, base, lane);
    const bool work = started || __ballot(hd) != 0;   // wave-uniform: this step is evaluated
    if (work && !r.full) r = reload_raw(a, base, lane);
    uint32_t sv = 0xFFFFFFFFu, ss = 0xFFFFFFFFu, gs0 = kNoSlot;
    uint4 rw = make_uint4(0, 0, 0, 0);
    if (valid && work) {
      sv = a.res_svc[r.res];
      ss = a.res_svc_str[r.res];
      consume(ss);   // (not used before the prefetch otherwise)
      if (sv < nsvc) {
        gs0 = gslot_of[sv];
        // route bytes only for a service with latency rules (in some chunk)
        if (gs0 != kNoSlot && r.route.len) rw = head16(a.arena, r.route.off, r.route.len);
      }
    }
    const uint64_t vmask = __ballot(valid);
    const uint64_t hmask = __ballot(hd);
    const bool in_range = base < range_end;
    if (in_range) {
      if (lane == 0 && a.win_heads) a.win_heads[base / kWave] = hmask;
      if (hmask) queue_heads(a, HQ, hn, hmask, hd, r.hi, r.lo, lane);
    }
    if (base + kWave < n) nx = load_raw(a, base + kWave, lane, work);   // prefetch the next step
    OSE_MARK("prefetch issued");
    uint64_t own;
    if (in_range) {
      if (!started) {
        if (!hmask) {   // still inside a trace an earlier wave owns
          base += kWave;
          if (base >= range_end) break;
          continue;
        }
        started = true;
        own = vmask & ~lanemask_lt(ffs64(hmask));
      } else {
        own = vmask;
      }
    } else {
      if (!open) break;
      own = vmask & (hmask ? lanemask_lt(ffs64(hmask)) : ~0ull);
    }
    const uint64_t segmask = (hmask & own) | (open ? 1ull : 0ull);
    const int last_own = fls64(own);
    bool cont_next = false;
    if (last_own == 63 && base + kWave < n) {
      bool h = false;
      if (lane == 63) h = r.ph != r.hi || r.pl != r.lo;   // lane 63 loaded the next step's first id
      cont_next = !lane_value((uint32_t)h, 63);
    }
    const bool mine = (own >> lane) & 1;
    const int sst = mine ? fls64(segmask & lanemask_le(lane)) : lane;
    const bool tail = mine && (lane == last_own || ((segmask >> (lane + 1)) & 1));
    const uint64_t tails = __ballot(tail);
    const int t0 = ffs64(tails);
    const bool seg0_cont = open;
    const bool single = t0 == last_own;
    const bool last_open = cont_next && !(single && seg0_cont);
    const int sst_last = lane_value((uint32_t)sst, last_own);
    const uint32_t hseg = mine ? (uint32_t)((segmask >> lane) & 1) : 1u;
    const uint32_t rst = (r.status & kStatusReset) ? 1u : 0u;
    const bool carried_tail = (lane == t0 && seg0_cont) || (lane == last_own && last_open);
    const bool ttail = tail && !carried_tail;   // the tail of a trace that opens and closes in this step
    const bool in_closed = mine && !(seg0_cont && lane <= t0) && !(last_open && lane >= sst_last);

    // ---- per-span words of every chunk ----
    const uint32_t gs = mine ? gs0 : kNoSlot;
    uint32_t err = mine && (r.status & ~kStatusReset) == OSE_STATUS_ERROR ? 1u : 0u;
    uint64_t st = 0, en = 0;
    if (gs != kNoSlot) {
      st = r.start;
      en = r.end;
    }
    uint64_t ep[K], svcb[K], lsat[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      const Cfg c = load_cfg(mcfg + coff[k]);
      ep[k] = svcb[k] = lsat[k] = 0;
      if (mine && ss < nsvc) svcb[k] = c.svc_bits[ss];
      if (gs != kNoSlot) {
        const uint32_t slot = c.svc_slot[sv];
        if (slot != kNoSlot) ep[k] = endpoint_bits_w(c, slot, a.arena, r.route, rw);
      }
    }
    // ---- latency state, once for every chunk: stretches of one trace and
    // one latency service (a chunk's slots are its services with rules: the
    // same stretches); the stretch tails' threshold tests per chunk ----
    uint64_t n_kmask = 0, smask = 0;
    Lat nxt{0, kInf, 0};
    bool rep = false;
    if (__ballot(gs != kNoSlot)) {
      const uint32_t pgs = dpp_mov<0x138>(kNoSlot, gs);
      const bool shead = !mine || hseg || pgs != gs;
      const uint32_t hs = shead ? 1u : 0u;
      const bool stail = mine && dpp_mov<0x130>(1u, hs) != 0;
      Lat v = gs != kNoSlot ? LAT_OF_SPAN(st, en, rst) : Lat{0u, kInf, 0ull};
      seg_lat_scan(hs, v);
      const bool lt = stail && (v.f & 2u);
      if (lt) {
#pragma unroll
        for (int k = 0; k < K; k++) {
          const Cfg c = load_cfg(mcfg + coff[k]);
          const uint32_t slot = c.svc_slot[sv];
          if (slot != kNoSlot) lsat[k] = latency_satisfied(c, slot, ~0ull, v.m, v.e);   // (ORed over the trace below)
        }
      }
      if (gs != kNoSlot) smask = 1ull << gs;
      if (seg0_cont) {   // the carried trace's stretches, in order
        for (uint64_t m0 = __ballot(lt && lane <= t0); m0; m0 &= m0 - 1) {
          const int L = ffs64(m0);
          const uint32_t ks = lane_value(gs, L);
          const Lat v0{lane_value(v.f, L), lane_value64(v.m, L), lane_value64(v.e, L)};
          if ((uint32_t)lane == ks) cur = lat_comb(cur, v0);
          c_kmask |= 1ull << ks;
        }
      }
      if (last_open) {   // the open trace's stretches, in order
        for (uint64_t m1 = __ballot(lt && lane >= sst_last); m1; m1 &= m1 - 1) {
          const int L = ffs64(m1);
          const uint32_t ks = lane_value(gs, L);
          const Lat v1{lane_value(v.f, L), lane_value64(v.m, L), lane_value64(v.e, L)};
          if ((uint32_t)lane == ks) nxt = lat_comb(nxt, v1);
          n_kmask |= 1ull << ks;
        }
      }
      uint32_t slo = (uint32_t)smask, shi = (uint32_t)(smask >> 32);
      seg_or_scan(hseg, slo, shi);
      const uint64_t psm = dpp_mov64<0x138, 0xF>(0ull, (uint64_t)slo | ((uint64_t)shi << 32));   // lane - 1's inclusive bits
      rep = in_closed && shead && !hseg && gs != kNoSlot && ((psm >> gs) & 1);
    }
    // ---- segmented ORs per trace: error, then each chunk's words ----
    seg_or_scan(hseg, err);
#pragma unroll
    for (int k = 0; k < K; k++) {
      seg_or_scan(hseg, ep[k], svcb[k], lsat[k]);
      lsat[k] = ttail ? lsat[k] & ep[k] : 0ull;
    }
    if (__ballot(rep)) {
      // a latency service with two or more stretches in a closed trace: its
      // monoid over the whole trace, and its rules' bits replaced per chunk
      uint32_t rlo = rep && gs < 32 ? 1u << gs : 0u, rhi = rep && gs >= 32 && gs != kNoSlot ? 1u << (gs - 32) : 0u;
      seg_or_scan(hseg, rlo, rhi);
      const uint64_t rm = (uint64_t)rlo | ((uint64_t)rhi << 32);
      for (uint64_t pend = __ballot(rep); pend;) {
        const uint32_t ks = lane_value(gs, ffs64(pend));
        const bool ink = gs == ks;
        pend &= ~__ballot(ink);
        Lat w = ink ? LAT_OF_SPAN(st, en, rst) : Lat{0u, kInf, 0ull};
        seg_lat_scan(hseg, w);
        if (ttail && ((rm >> ks) & 1)) {
#pragma unroll
          for (int k = 0; k < K; k++) {
            const Cfg c = load_cfg(mcfg + coff[k]);
            const uint32_t slot = c.svc_slot[gsvc[ks]];
            if (slot != kNoSlot)
              lsat[k] = (lsat[k] & ~c.slot_rules[slot]) | ((w.f & 2u) ? latency_satisfied(c, slot, ep[k], w.m, w.e) : 0ull);
          }
        }
      }
    }
    // ---- queue the carried trace (if it closes) and this step's traces ----
    const bool cont_close = seg0_cont && !(single && cont_next);
    const uint64_t qmask = __ballot(ttail);
    const uint32_t ncl = cont_close ? 1u : 0u, nq = __popcll(qmask);
    if (qn + ncl + nq > (uint32_t)kQ) flush_multi<K>(a, mcfg, coff, wlk, Q, qn, lane);
    const uint32_t qcl = qn;
    const uint32_t qe = qn + ncl + __popcll(qmask & lanemask_lt(lane));
    if (cont_close && lane == 0) {
      Q.err[qcl] = c_err | lane_value(err, t0);
      Q.hi[qcl] = c_hi;
      Q.lo[qcl] = c_lo;
      Q.pos[qcl] = (uint32_t)c_pos;
      Q.len[qcl] = (uint32_t)(base + t0 + 1 - c_pos);
    }
    if (ttail) {
      Q.err[qe] = err;
      Q.hi[qe] = r.hi;
      Q.lo[qe] = r.lo;
      Q.pos[qe] = (uint32_t)(base + sst);
      Q.len[qe] = (uint32_t)(lane - sst + 1);
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
      if (cont_close) {
        const Cfg c = load_cfg(mcfg + coff[k]);
        const uint64_t EP = c_ep[k] | lane_value64(ep[k], t0);
        uint64_t s_l = 0;
        if ((c_kmask >> lane) & 1) {
          const uint32_t slot = c.svc_slot[gsvc[lane]];
          if (slot != kNoSlot) s_l = latency_satisfied(c, slot, EP, cur.m, cur.e);
        }
        s_l = wave_or64(s_l);
        if (lane == 0) {
          Q.ep[k][qcl] = EP;
          Q.lsat[k][qcl] = s_l;
          Q.svc[k][qcl] = c_svc[k] | lane_value64(svcb[k], t0);
        }
      }
      if (ttail) {
        Q.ep[k][qe] = ep[k];
        Q.lsat[k][qe] = lsat[k];
        Q.svc[k][qe] = svcb[k];
      }
      // ---- carry into the next step ----
      if (last_open) {
        c_ep[k] = lane_value64(ep[k], last_own);
        c_svc[k] = lane_value64(svcb[k], last_own);
      } else if (seg0_cont && single && cont_next) {
        c_ep[k] |= lane_value64(ep[k], t0);
        c_svc[k] |= lane_value64(svcb[k], t0);
      }
    }
    qn += ncl + nq;
    if (cont_close) {
      open = false;
      cur = Lat{0, kInf, 0};
      c_kmask = 0;
    }
    if (last_open) {
      open = true;
      c_pos = base + sst_last;
      c_hi = lane_value64(r.hi, sst_last);
      c_lo = lane_value64(r.lo, sst_last);
      c_err = lane_value(err, last_own);
      cur = nxt;
      c_kmask = n_kmask;
    } else if (seg0_cont && single && cont_next) {
      c_err |= lane_value(err, t0);
    }
    base += kWave;
    if (!open && base >= range_end) break;
  }
  flush_multi<K>(a, mcfg, coff, wlk, Q, qn, lane);
  flush_heads(a, HQ, hn, lane);
}

// ---- long runs ------------------------------------------------------------------
// A run the fast path listed (kTraceRuns; still open long_steps steps past
// its owner's windows) is one trace.  Zipf run lengths put most of a batch's
// spans in a few runs, so a run is not one workgroup's work (one workgroup
// per run: C5 0.98 ms, most of it the few workgroups holding 50k-span runs):
//  - trace_long_plan_kernel finds each run's end from the window head masks
//    and cuts it into pieces of at most kLongPiece spans;
//  - trace_long_kernel's waves take the pieces in turn, each on its own (no
//    workgroup barrier): a piece's per-span contributions exactly as
//    trace_eval_kernel computes them, the latency monoid reduced in lane
//    order, then step order; a one-piece run is decided there, a piece of a
//    longer run leaves its partial in long_part;
//  - trace_long_decide_kernel combines each longer run's partials in piece
//    order, decides, and writes the run's keep bytes.
// The partials cross workgroups (and XCDs) through the kernel boundary: a
// release / acquire pair per piece inside one kernel writes back the L2 each
// time (2.8 ms at 1024-span pieces).  C5: 0.98 -> 0.66 ms (profiles/r5l_long_pieces.txt).
// the columns of one span of a long run (loaded two steps ahead)
struct LongRaw {
  uint32_t res, status;
  uint64_t st, en, am, rm, svm;
  ose_strref rt;
};
__device__ __forceinline__ LongRaw long_raw(const TraceKernelArgs& a, const SampCfgDev* h, uint64_t p, uint64_t hi) {
  LongRaw r{};
  if (p >= hi) return r;
  r.res = a.resource[p];
  r.status = a.status[p];
  if (a.start) {
    r.st = a.start[p];
    r.en = a.end[p];
  }
  if (a.attr_match) r.am = chunk_attr_bits(a.attr_match, a.attr_stride, a.attr_words, h, p);
  if (a.svc_match) r.svm = a.svc_match[p];
  if (a.route_match) r.rm = a.route_match[p];
  else if (a.route) r.rt = a.route[p];
  return r;
}

// one wave per listed run: its end (the first head after it), its pieces;
// a workgroup's 16 runs take their piece and partial ranges with one atomic
// each (per-wave atomics on two counters serialised 0.1 ms on C5)
constexpr int kPlanWaves = 16;
__global__ __launch_bounds__(kPlanWaves * kWave) void trace_long_plan_kernel(TraceKernelArgs a) {
  __shared__ uint32_t s_np[kPlanWaves];
  __shared__ uint32_t s_q, s_p;
  const uint32_t nl = __hip_atomic_load(a.n_long, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int lane = threadIdx.x & 63;
  const uint32_t wv = threadIdx.x >> 6;
  for (uint32_t r0 = blockIdx.x * kPlanWaves; r0 < nl; r0 += gridDim.x * kPlanWaves) {
    const uint32_t r = r0 + wv;
    uint64_t pos = 0, end = a.n_spans;
    uint32_t np = 0;
    if (r < nl) {
      pos = a.long_runs[r];
      const uint32_t w0 = (uint32_t)(pos / kWave);
      const uint64_t m0 = a.win_heads[w0] & ~lanemask_le((int)(pos % kWave));
      if (m0) {
        end = (uint64_t)w0 * kWave + ffs64(m0);
      } else {
        for (uint64_t wb = (uint64_t)w0 + 1; wb < a.n_windows; wb += kWave) {
          const uint64_t w = wb + lane;
          const uint64_t h = w < a.n_windows ? a.win_heads[w] : 0ull;
          const uint64_t b = __ballot(h != 0);
          if (b) {
            const int l = (int)ffs64(b);
            end = (wb + l) * kWave + ffs64(lane_value64(h, l));
            break;
          }
        }
      }
      np = (uint32_t)((end - pos + kLongPiece - 1) / kLongPiece);
    }
    if (lane == 0) s_np[wv] = np;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tq = 0, tp = 0;
      for (int w = 0; w < kPlanWaves; w++) {
        tq += s_np[w];
        tp += s_np[w] > 1 ? s_np[w] : 0u;
      }
      s_q = tq ? atomicAdd(a.n_long + 1, tq) : 0u;
      s_p = tp ? atomicAdd(a.n_long + 3, tp) : 0u;
    }
    __syncthreads();
    if (r < nl) {
      uint32_t q0 = s_q, pb = s_p;
      for (uint32_t w = 0; w < wv; w++) {
        q0 += s_np[w];
        pb += s_np[w] > 1 ? s_np[w] : 0u;
      }
      if (lane == 0) a.long_meta[r] = make_uint4((uint32_t)end, np, np > 1 ? pb : 0u, 0u);
      for (uint32_t k = lane; k < np; k += kWave) a.long_pieces[q0 + k] = make_uint2(r, k);
    }
    __syncthreads();   // s_np / s_q / s_p are read before the next round's writes
  }
}

constexpr int kLWaves = 8;
constexpr int kLThreads = kLWaves * kWave;
struct LongPart {   // kLongPartBytes
  uint64_t m[kWave], e[kWave];
  uint32_t f[kWave];
  uint64_t ep, svc, kmask;
  uint32_t err;
  uint32_t _pad[9];   // 21 cache lines
};
static_assert(sizeof(LongPart) == kLongPartBytes, "long-run partial layout");
// keep bytes [x0, x1) = k, 16-byte stores in the aligned middle
__device__ __forceinline__ void long_keep_fill(uint8_t* keep, uint64_t x0, uint64_t x1, uint8_t k, int lane) {
  const uint64_t b = reinterpret_cast<uintptr_t>(keep);
  const uint64_t a0 = min(x1, ((b + x0 + 15) & ~15ull) - b), a1 = max(a0, ((b + x1) & ~15ull) - b);
  for (uint64_t x = x0 + lane; x < a0; x += kWave) keep[x] = k;
  const uint32_t k4 = k * 0x01010101u;
  for (uint64_t x = a0 + 16ull * lane; x < a1; x += 16ull * kWave) *reinterpret_cast<uint4*>(keep + x) = make_uint4(k4, k4, k4, k4);
  for (uint64_t x = a1 + lane; x < x1; x += kWave) keep[x] = k;
}
// a long run's decision (wave-wide: lane k holds latency slot k's monoid)
// and its keep bytes
__device__ __forceinline__ void long_decide(const TraceKernelArgs& a, const Cfg& c, int lane, uint64_t pos, uint64_t end,
                                            uint32_t E, uint64_t EP, uint64_t SV, uint64_t K, const Lat& tot) {
  uint64_t s_l = 0;
  if ((K >> lane) & 1) s_l = latency_satisfied(c, (uint32_t)lane, EP, tot.m, tot.e);
  s_l = wave_or64(s_l);
  uint32_t dk32 = 0;
  if (lane == 0) {
    const uint4 t = reinterpret_cast<const uint4*>(a.tid)[pos];
    uint8_t dk = 0, dl = 0;
    double dr = 0;
    decide_at(a, c, pos, E, EP, s_l, SV,
              trace_uniform((uint64_t)t.x | ((uint64_t)t.y << 32), (uint64_t)t.z | ((uint64_t)t.w << 32), a.seed), dk, dl,
              dr);
    write_rec(a, pos, dk, dl, dr);
    dk32 = dk;
  }
  long_keep_fill(a.keep, pos, end, (uint8_t)lane_value(dk32, 0), lane);
}
// Each wave takes pieces in turn, on its own (no workgroup barrier after
// the table copy): a piece's latency chain overlaps the other waves' folds
__global__ __launch_bounds__(kLThreads) void trace_long_kernel(TraceKernelArgs a) {
  const uint32_t npieces = __hip_atomic_load(a.n_long + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (blockIdx.x * kLWaves >= npieces) return;
  __shared__ __attribute__((aligned(16))) uint8_t cfg_lds[kSampCfgLds];
  {
    // (written out: copy_cfg_to_lds here renumbers this kernel's spill lanes)
    const uint32_t nb = cfg_lds_copy_bytes(a.cfg);
    for (uint32_t k = threadIdx.x * 16; k < nb; k += kLThreads * 16)
      *reinterpret_cast<uint4*>(cfg_lds + k) = *reinterpret_cast<const uint4*>(a.cfg + k);
    __syncthreads();   // every wave reads the tables (n_services, n_lat below) after the copy
  }
  const Cfg c = load_cfg(cfg_lds);
  const int lane = threadIdx.x & 63;
  const uint32_t nsvc = c.h->n_services;
  const bool want_route = c.h->n_lat && !a.route_match && a.route;
  const uint32_t stride = gridDim.x * kLWaves;
  for (uint32_t q = blockIdx.x * kLWaves + (threadIdx.x >> 6); q < npieces; q += stride) {
    const uint2 pk = a.long_pieces[q];
    const uint4 meta = a.long_meta[pk.x];   // {end, pieces, first partial, pieces done}
    const uint64_t pos = a.long_runs[pk.x], end = meta.x;
    const uint64_t lo = pos + (uint64_t)pk.y * kLongPiece, hi = min(end, lo + kLongPiece);
    uint32_t err = 0;
    uint64_t ep_acc = 0, svc_acc = 0, kmask = 0;
    Lat cur{0, kInf, 0};   // lane k: latency slot k
    // two steps of columns in flight, the service ids of the next step
    // gathered a step ahead: a step's route head waits on nothing of its own
    LongRaw r0 = long_raw(a, c.h, lo + lane, hi), r1 = long_raw(a, c.h, lo + kWave + lane, hi);
    uint32_t nsv = 0xFFFFFFFFu, nss = 0xFFFFFFFFu;
    if (lo + lane < hi) {
      nsv = a.res_svc[r0.res];
      nss = a.res_svc_str[r0.res];
    }
    for (uint64_t base = lo; base < hi; base += kWave) {
      const uint64_t p = base + lane;
      const bool valid = p < hi;
      const LongRaw r = r0;
      const uint32_t sv = nsv, ss = nss;
      uint4 rw = make_uint4(0, 0, 0, 0);
      if (valid && want_route && r.rt.len && sv < nsvc && c.svc_slot[sv] != kNoSlot)
        rw = head16(a.arena, r.rt.off, r.rt.len);
      r0 = r1;
      if (base + 2 * kWave < hi) r1 = long_raw(a, c.h, p + 2 * kWave, hi);
      if (p + kWave < hi) {
        nsv = a.res_svc[r0.res];
        nss = a.res_svc_str[r0.res];
      }
      uint32_t slot = kNoSlot;
      uint64_t st = 0, en = 0;
      const uint32_t rst = (r.status & kStatusReset) ? 1u : 0u;
      if (valid) {
        err |= (r.status & ~kStatusReset) == OSE_STATUS_ERROR;
        if (a.svc_match) {
          svc_acc |= r.svm;
        } else {
          if (ss < nsvc) svc_acc |= c.svc_bits[ss];
          svc_acc |= r.am;
        }
        if (sv < nsvc) {
          slot = c.svc_slot[sv];
          if (slot != kNoSlot) {
            ep_acc |= a.route_match ? r.rm & c.slot_rules[slot] : endpoint_bits_w(c, slot, a.arena, r.rt, rw);
            st = r.st;
            en = r.en;
          }
        }
      }
      uint64_t pend = __ballot(slot != kNoSlot);
      while (pend) {
        const uint32_t ks = lane_value(slot, ffs64(pend));
        const bool ink = slot == ks;
        pend &= ~__ballot(ink);
        Lat v = ink ? LAT_OF_SPAN(st, en, rst) : Lat{0u, kInf, 0ull};
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {   // lane-order reduction into lane 0
          Lat o;
          o.f = __shfl_down(v.f, d, kWave);
          o.m = __shfl_down(v.m, d, kWave);
          o.e = __shfl_down(v.e, d, kWave);
          if ((lane & (2 * d - 1)) == 0) v = lat_comb(v, o);
        }
        const Lat v0{lane_value(v.f, 0), lane_value64(v.m, 0), lane_value64(v.e, 0)};
        if ((uint32_t)lane == ks) cur = lat_comb(cur, v0);
        kmask |= 1ull << ks;
      }
    }
    uint32_t E = __ballot(err != 0) ? 1u : 0u;
    uint64_t EP = wave_or64(ep_acc), SV = wave_or64(svc_acc), K = kmask;
    Lat tot = cur;
    if (meta.y > 1) {   // trace_long_decide_kernel combines the run's partials
      LongPart* part = reinterpret_cast<LongPart*>(a.long_part + (size_t)kLongPartBytes * (meta.z + pk.y));
      part->m[lane] = tot.m;
      part->e[lane] = tot.e;
      part->f[lane] = tot.f;
      if (lane == 0) {
        part->ep = EP;
        part->svc = SV;
        part->kmask = K;
        part->err = E;
      }
      continue;
    }
    long_decide(a, c, lane, pos, end, E, EP, SV, K, tot);
  }
}

// one wave per run of several pieces: its partials in piece order, the
// decision, the run's keep bytes
__global__ __launch_bounds__(kPlanWaves * kWave) void trace_long_decide_kernel(TraceKernelArgs a) {
  const uint32_t nl = __hip_atomic_load(a.n_long, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (blockIdx.x * kPlanWaves >= nl) return;
  __shared__ __attribute__((aligned(16))) uint8_t cfg_lds[kSampCfgLds];
  copy_cfg_to_lds<kPlanWaves * kWave>(cfg_lds, a.cfg);
  __syncthreads();
  const Cfg c = load_cfg(cfg_lds);
  const int lane = threadIdx.x & 63;
  for (uint32_t r = blockIdx.x * kPlanWaves + (threadIdx.x >> 6); r < nl; r += gridDim.x * kPlanWaves) {
    const uint4 meta = a.long_meta[r];
    if (meta.y <= 1) continue;
    uint32_t E = 0;
    uint64_t EP = 0, SV = 0, K = 0;
    Lat tot{0, kInf, 0};
    const LongPart* pp = reinterpret_cast<const LongPart*>(a.long_part + (size_t)kLongPartBytes * meta.z);
    for (uint32_t k0 = 0; k0 < meta.y; k0 += 4) {   // piece order, 4 partials' loads in flight
      uint64_t kk[4], m[4], e[4];
      uint32_t f[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const LongPart& q = pp[k0 + j < meta.y ? k0 + j : k0];
        kk[j] = k0 + j < meta.y ? q.kmask : 0ull;
        E |= q.err;
        EP |= q.ep;
        SV |= q.svc;
        f[j] = q.f[lane];
        m[j] = q.m[lane];
        e[j] = q.e[lane];
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        K |= kk[j];
        if ((kk[j] >> lane) & 1) tot = lat_comb(tot, Lat{f[j], m[j], e[j]});
      }
    }
    long_decide(a, c, lane, a.long_runs[r], meta.x, E, EP, SV, K, tot);
  }
}

// The endpoint bits of every span under one rule chunk's tables read from
// HBM (a chunk whose route bytes spill past the kernels' LDS copy): the
// plane the trace stage and the pack then take as route_match
__global__ __launch_bounds__(256) void endpoint_plane_kernel(const uint8_t* cfg, const uint32_t* resource,
                                                             const uint32_t* res_svc, const ose_strref* route,
                                                             const uint8_t* arena, uint64_t n, uint64_t* out) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const Cfg c = load_cfg(cfg);
  const uint32_t sv = res_svc[resource[j]];
  uint64_t ep = 0;
  if (sv < c.h->n_services) {
    const uint32_t slot = c.svc_slot[sv];
    if (slot != kNoSlot) ep = endpoint_bits(c, slot, arena, route[j]);
  }
  out[j] = ep;
}

// One workgroup per fingerprint bucket: its entries into an LDS hash set; an
// entry met twice (or a bucket past its capacity) sets *dup
__global__ __launch_bounds__(256) void trace_dup_check_kernel(TraceKernelArgs a) {
  constexpr uint32_t kSet = 2 * kDupBucketCap;
  static_assert(kSet == 2048, "the set hash takes at most 11 bits");
  __shared__ uint64_t set[kSet];
  __shared__ uint32_t found;
  const uint32_t bk = blockIdx.x;
  const uint32_t c = a.dup_bkt_count[bk];
  if (c <= 1) return;
  if (c > kDupBucketCap) {
    if (threadIdx.x == 0) atomicOr(a.dup, 1u);
    return;
  }
  // the set: the power of two >= 2c (>= 256), so a bucket of ~c entries
  // clears ~2c slots instead of all kSet
  uint32_t bits = 8;
  while ((1u << bits) < 2 * c) bits++;
  const uint32_t nset = 1u << bits;   // <= kSet (c <= kDupBucketCap)
  for (uint32_t k = threadIdx.x; k < nset; k += 256) set[k] = 0ull;
  if (threadIdx.x == 0) found = 0;
  __syncthreads();
  const uint64_t* e = a.dup_bkt + (uint64_t)bk * kDupBucketCap;
  bool hit = false;
  for (uint32_t k = threadIdx.x; k < c; k += 256) {
    const uint64_t v = e[k];   // never 0
    uint32_t s = ((uint32_t)v * 0x9E3779B1u) >> (32 - bits);
    for (uint32_t probes = 0; probes < nset; probes++) {
      const uint64_t old = atomicCAS((unsigned long long*)&set[s], 0ull, (unsigned long long)v);
      if (old == 0) break;
      if (old == v) { hit = true; break; }
      s = (s + 1) & (nset - 1);
    }
  }
  if (hit) found = 1;
  __syncthreads();
  if (threadIdx.x == 0 && found) atomicOr(a.dup, 1u);
}

// Chunk-local service ids (sampling_host.cpp local_service_ids)
__global__ __launch_bounds__(256) void svc_translate_kernel(const uint32_t* map, uint32_t n_global, const uint32_t* in1,
                                                            const uint32_t* in2, uint32_t* out1, uint32_t* out2,
                                                            uint64_t n) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const uint32_t a = in1[r], b = in2[r];
  out1[r] = a < n_global ? map[a] : 0xFFFFFFFFu;
  out2[r] = b < n_global ? map[b] : 0xFFFFFFFFu;
}

}  // namespace

void launch_trace_eval(const TraceKernelArgs& a, hipStream_t st) {
  const uint32_t per_block = kTWaves * a.win_per_wave;
  const uint32_t blocks = (a.n_windows + per_block - 1) / per_block;
  if (a.n_multi) {   // every rule chunk in one pass (run_sampling checks the conditions)
    if (a.n_multi == 2)
      hipLaunchKernelGGL((trace_multi_kernel<2>), dim3(blocks), dim3(kTThreads), a.cfg_lds_bytes, st, a);
    else
      hipLaunchKernelGGL((trace_multi_kernel<3>), dim3(blocks), dim3(kTThreads), a.cfg_lds_bytes, st, a);
    return;
  }
  if (a.mode == kTraceRuns && !a.svc_match && !a.route_match && !a.attr_match && (OSE_DIAG || !a.ablate)) {
    const bool chunk = a.fold_in || a.fold_out;
    if (a.narrow && chunk)
      hipLaunchKernelGGL((trace_eval_kernel<true, true, true>), dim3(blocks), dim3(kTThreads), 0, st, a);
    else if (a.narrow)
      hipLaunchKernelGGL((trace_eval_kernel<true, true, false>), dim3(blocks), dim3(kTThreads), 0, st, a);
    else if (chunk)
      hipLaunchKernelGGL((trace_eval_kernel<true, false, true>), dim3(blocks), dim3(kTThreads), 0, st, a);
    else
      hipLaunchKernelGGL((trace_eval_kernel<true, false, false>), dim3(blocks), dim3(kTThreads), 0, st, a);
  } else {
    hipLaunchKernelGGL((trace_eval_kernel<false, false, false>), dim3(blocks), dim3(kTThreads), 0, st, a);
  }
}
void launch_trace_dup_check(const TraceKernelArgs& a, hipStream_t st) {
  if (a.dup_bkt) hipLaunchKernelGGL(trace_dup_check_kernel, dim3(1u << a.dup_bkt_bits), dim3(256), 0, st, a);
}
void launch_trace_long(const TraceKernelArgs& a, hipStream_t st, uint32_t known_runs) {
  // known_runs: the listed-run count the host read (host-gated form); else
  // grids for the most runs the fast path can list, workgroups past the
  // device counts exit
  const uint64_t most = known_runs ? known_runs : a.n_spans / ((uint64_t)a.long_steps * kWave) + 1;
  hipLaunchKernelGGL(trace_long_plan_kernel, dim3((uint32_t)std::min<uint64_t>((most + kPlanWaves - 1) / kPlanWaves, 1024)),
                     dim3(kPlanWaves * kWave), 0, st, a);
  const uint64_t pieces = most + a.n_spans / kLongPiece + 1;
  hipLaunchKernelGGL(trace_long_kernel, dim3((uint32_t)std::min<uint64_t>((pieces + kLWaves - 1) / kLWaves, 1024)),
                     dim3(kLThreads), 0, st, a);
  hipLaunchKernelGGL(trace_long_decide_kernel, dim3((uint32_t)std::min<uint64_t>((most + kPlanWaves - 1) / kPlanWaves, 1024)),
                     dim3(kPlanWaves * kWave), 0, st, a);
}
void launch_endpoint_plane(const uint8_t* cfg, const uint32_t* resource, const uint32_t* res_svc, const ose_strref* route,
                           const uint8_t* arena, uint64_t n, uint64_t* out, hipStream_t st) {
  if (n) hipLaunchKernelGGL(endpoint_plane_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, cfg, resource,
                            res_svc, route, arena, n, out);
}
void launch_svc_translate(const uint32_t* map, uint32_t n_global, const uint32_t* in1, const uint32_t* in2, uint32_t* out1,
                          uint32_t* out2, uint64_t n, hipStream_t st) {
  if (n) hipLaunchKernelGGL(svc_translate_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, map, n_global, in1,
                            in2, out1, out2, n);
}

}  // namespace ose
