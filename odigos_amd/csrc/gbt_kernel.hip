// gbt_kernel.hip — the GPU-resident groupbytrace store.
//
// Spans wait in HBM until their trace's wait_duration has passed, then
// leave as one batch in which every released trace is contiguous: the
// batch the three processors see is the sequence of per-trace calls
// groupbytrace makes, and SAMPLE with OSE_GROUP_TRACE_ID decides each trace
// as its own call would.
//
// State (gbt_host.cpp owns the buffers and the host-side clock):
//   * traces are numbered in creation order (seq, 64-bit); the ring of
//     num_traces ids (contrib's ringBuffer) is ring_tid[seq % num_traces],
//     so a trace created num_traces creations after another evicts it;
//     with num_workers W > 1 each worker has its own ring of num_traces / W
//     ids (contrib's eventMachineWorker.buffer): a trace's worker is
//     fnv64(id) % W, its number q within the worker is kept in tinfo, and
//     it is evicted by its worker's trace number q + num_traces / W;
//   * the id -> seq table persists across adds (tombstones: an id whose
//     trace is gone reclaims its own slot; the table is re-inserted from the
//     live traces only when it grows or tombstones fill half of it); the
//     batch's spans look themselves up, and ids without a live trace start
//     new traces, numbered in the order of their first span in the batch;
//   * spans go to a pool ring in arrival order (columns + a string block in
//     an arena ring), scopes to a scope ring (the fragment's resource and
//     scope columns);
//   * a release takes the traces created before now - wait_duration: a
//     contiguous seq range.  Its spans are flagged in the pool window,
//     compacted, stably sorted by seq (arrival order kept inside a trace)
//     and gathered into fresh columns, one resource and one scope per
//     fragment (a run of one trace from one scope of one added batch).
//
// A store on an engine with the odigossqldboperationprocessor section
// (GbtArgs::sql) also carries db_flags, db_query and res_sql_ok.  The query
// bytes are the last string of the span's block.  Routes and paths are a few
// tens of bytes and move one lane per span; a query is longer (up to KiBs),
// so the SQL instances move bytes a wave at a time (gbt_query_copy_kernel on
// the add, gbt_block_copy_kernel on the release).  The kernels are templates
// on kSql: the <false> instances are the kernels of a store without the
// section and never read the three columns.
//
// A store fed by ose_gbt_add_otlp (GbtArgs::otlp, template parameter kOtlp)
// also keeps what ose_otlp_encode needs to write a released span out again:
// a span's block starts with its Span message (every ref of the block shifts
// by the message's length; the query stays last), and every added scope has a
// header block in the ring, after the add's span blocks: its ResourceSpans
// payload without the scope_spans fields, then its ScopeSpans payload without
// the spans fields.  The release lays out, per fragment, the header block and
// then the spans' blocks, and writes the layout arrays the encoder reads.
// Messages are a few hundred bytes: gbt_msg_copy_kernel (add) and
// gbt_block_copy_kernel<true> (release) move them a wave at a time with
// 16-byte stores.  Offsets are 32-bit scans; gbt_total_kernel sums the same
// lengths in 64 bits, and that total decides refusals and sizes.  The
// <., false> instances are the kernels of a columns-fed store.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "pb_device.hpp"      // Rd: the header blocks' top-level fields (OTLP mode)
#include "trace_device.hpp"   // tid_hash: the trace table's hash

namespace ose {

namespace {
constexpr int kGbtThreads = 256;
constexpr uint64_t kUnset = ~0ull;

// contrib's workerIndexForTraceID: FNV-1 (64-bit) over the id's 16 bytes,
// modulo the workers (ids are {hi, lo}, big-endian)
__device__ __forceinline__ uint32_t gbt_worker(uint64_t hi, uint64_t lo, uint32_t n_workers) {
  uint64_t h = 14695981039346656037ull;
#pragma unroll
  for (int b = 0; b < 16; b++) {
    h *= 1099511628211ull;
    h ^= ((b < 8 ? hi : lo) >> (56 - 8 * (b & 7))) & 0xFFu;
  }
  return (uint32_t)(h % n_workers);
}

// a trace whose worker has numbered worker_cap more traces after it: the
// last of them took its ring slot (one worker: the contiguous eviction is in
// live_lo instead)
__device__ __forceinline__ bool gbt_evicted(const GbtArgs& a, uint64_t seq) {
  if (a.n_workers <= 1) return false;
  const uint64_t t = a.tinfo[seq % a.ring_n];
  return a.wcnt[t >> 40] > (t & ((1ull << 40) - 1)) + a.worker_cap;
}

// The id table persists across adds.  A slot holds an id and the creation
// number of its newest trace; the trace is live for an added span iff that
// number is in [live_lo, live_hi) (not released, evicted or expired).  A
// slot whose trace is no longer live stays as a tombstone: lookups of other
// ids probe past it, and its own id takes it back (reclaim) when it comes
// again.  The host bumps the epoch and re-inserts the live traces only when
// the table grows or tombstones fill half of it, so an add costs O(batch),
// not O(traces waiting).
//
// Slots are published with the trace table's protocol (trace_slow_kernel.hip table_insert): a
// stale-epoch slot is claimed BUSY, its fields stored with agent-scope
// stores, drained, then READY.

// rebuild: one live trace per id (an id's expired instance is outside
// [live_lo, live_hi), so each id occurs at most once; the newest wins anyway)
__device__ void gbt_put(const GbtArgs& a, uint64_t hi, uint64_t lo, uint64_t seq) {
  const uint32_t busy = (a.epoch << 2) | 1u, ready = (a.epoch << 2) | 2u;
  uint64_t h = tid_hash(hi, lo) & a.table_mask;
  uint32_t probes = 0, spins = 0;
  for (;;) {
    GbtSlot* s = &a.table[h];
    const uint32_t st = __hip_atomic_load(&s->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((st >> 2) != a.epoch) {
      uint32_t expect = st;
      if (__hip_atomic_compare_exchange_strong(&s->state, &expect, busy, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        __hip_atomic_store(&s->hi, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->lo, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->first, ~0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&s->state, ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
      }
      continue;
    }
    if ((st & 3u) != 2u) {
      if (++spins > (1u << 20)) {
        atomicOr(a.error, kGbtErrSpin);
        return;
      }
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    if (__hip_atomic_load(&s->hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == hi &&
        __hip_atomic_load(&s->lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == lo) {
      __hip_atomic_fetch_max(&s->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    h = (h + 1) & a.table_mask;
    if (++probes > a.table_mask) {
      atomicOr(a.error, kGbtErrProbe);
      return;
    }
  }
}

// lookup of an added span: the slot of its id, which holds either a live
// trace or (claimed or reclaimed for this add) kGbtUnset | add_gen with the
// smallest batch position of the id in `first`.  UINT64_MAX on failure.
__device__ uint64_t gbt_lookup(const GbtArgs& a, uint64_t hi, uint64_t lo, uint32_t pos) {
  const uint32_t busy = (a.epoch << 2) | 1u, ready = (a.epoch << 2) | 2u;
  const uint64_t mine = kGbtUnset | a.add_gen;
  uint64_t h = tid_hash(hi, lo) & a.table_mask;
  uint32_t probes = 0, spins = 0;
  for (;;) {
    GbtSlot* s = &a.table[h];
    const uint32_t st = __hip_atomic_load(&s->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((st >> 2) != a.epoch) {   // empty: the id is not in the table
      uint32_t expect = st;
      if (__hip_atomic_compare_exchange_strong(&s->state, &expect, busy, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        __hip_atomic_store(&s->hi, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->lo, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->seq, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->first, pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&s->state, ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return h;
      }
      continue;
    }
    if ((st & 3u) != 2u) {   // another lane is publishing or reclaiming this slot
      if (++spins > (1u << 20)) {
        atomicOr(a.error, kGbtErrSpin);
        return ~0ull;
      }
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    if (__hip_atomic_load(&s->hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != hi ||
        __hip_atomic_load(&s->lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != lo) {
      h = (h + 1) & a.table_mask;   // another id (live or a tombstone)
      if (++probes > a.table_mask) {
        atomicOr(a.error, kGbtErrProbe);
        return ~0ull;
      }
      continue;
    }
    const uint64_t seq = __hip_atomic_load(&s->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seq == mine) {   // numbered by this add
      atomicMin(&s->first, pos);
      return h;
    }
    if (seq < kGbtUnset && seq >= a.live_lo && seq < a.live_hi && !gbt_evicted(a, seq)) return h;   // a live trace
    // the id's last trace is gone (released, evicted, expired) or an earlier
    // add failed while numbering it: the id starts a new trace in this slot
    uint32_t expect = st;
    if (__hip_atomic_compare_exchange_strong(&s->state, &expect, busy, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT)) {
      if (__hip_atomic_load(&s->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == mine) {
        atomicMin(&s->first, pos);   // reclaimed by another lane between our reads
      } else {
        // first before seq, drained between them: a lane that read the state
        // as READY before this CAS may still read seq; once it sees `mine`
        // its atomicMin must land after this store, not under it
        __hip_atomic_store(&s->first, pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&s->seq, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(&s->state, ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return h;
    }
  }
}

// ---- add -------------------------------------------------------------------

// the live traces [live_lo, live_hi) back into a fresh epoch of the table
__global__ __launch_bounds__(kGbtThreads) void gbt_rebuild_kernel(GbtArgs a) {
  for (uint64_t s = a.live_lo + (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x; s < a.live_hi;
       s += (uint64_t)gridDim.x * kGbtThreads) {
    if (gbt_evicted(a, s)) continue;
    const uint64_t r = s % a.ring_n;
    gbt_put(a, a.ring_tid[2 * r], a.ring_tid[2 * r + 1], s);
  }
}

// every span of the batch: its table slot
__global__ __launch_bounds__(kGbtThreads) void gbt_lookup_kernel(GbtArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (i >= a.n) return;
  a.slot_of[i] = gbt_lookup(a, a.cols.trace_id[2 * i], a.cols.trace_id[2 * i + 1], (uint32_t)i);
}

// OSE_GBT_SQL_PERLANE (an A/B build, odigos_amd/build.py --variant): the SQL
// instances move the query bytes as the routes are moved, one lane per span
// and a byte per iteration, and the two wave copies are not launched.  It is
// the baseline the wave copies were measured against.
#ifdef OSE_GBT_SQL_PERLANE
constexpr bool kWaveCopy = false;
#else
constexpr bool kWaveCopy = true;
#endif

// the span's query ref in the added batch: read only under OSE_DB_HAS_QUERY
__device__ __forceinline__ ose_strref gbt_batch_query(const ose_columns& c, uint64_t i) {
  if (c.db_flags && (c.db_flags[i] & OSE_DB_HAS_QUERY)) return c.db_query[i];
  return ose_strref{0, 0};
}

// creators (the first span of each new trace) and each span's string block length
template <bool kSql, bool kOtlp>
__global__ __launch_bounds__(kGbtThreads) void gbt_creator_kernel(GbtArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t h = a.slot_of[i];
  uint32_t f = 0;
  if (h != ~0ull) {
    const GbtSlot& s = a.table[h];
    f = s.seq == (kGbtUnset | a.add_gen) && s.first == (uint32_t)i;
  }
  a.flag[i] = f;
  const ose_columns& c = a.cols;
  uint32_t len = 0;
  if (c.route) len += c.route[i].len;
  if (c.path) len += c.path[i].len;
  for (uint32_t k = 0; k < a.n_attr_keys; k++)
    if (c.attr_type[(uint64_t)k * a.n + i] == OSE_ATTR_STR) len += (uint32_t)(c.attr_val[(uint64_t)k * a.n + i] >> 32);
  if constexpr (kSql) len += gbt_batch_query(c, i).len;
  if constexpr (kOtlp) len += (uint32_t)(a.otlp.span_ref[i] >> 32);   // the message leads the block
  a.strlen[i] = len;
}

// the batch's strings do not fit the arena ring: nothing of the batch is
// stored (no trace numbered, no ring slot overwritten) and the add fails
// (OTLP mode: blocks and header blocks, summed in 64 bits)
template <bool kOtlp = false>
__device__ __forceinline__ bool gbt_batch_refused(const GbtArgs& a) {
  if constexpr (kOtlp) return a.otlp.total64[0] > a.arena_room || (a.error[0] & kGbtErrHeader);
  return (uint64_t)a.totals[1] > a.arena_room;
}

// new traces numbered in first-appearance order; the ring remembers their ids
template <bool kOtlp>
__global__ __launch_bounds__(kGbtThreads) void gbt_assign_kernel(GbtArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (gbt_batch_refused<kOtlp>(a)) {
    if (i == 0) atomicOr(a.error, kGbtErrRefused);
    return;
  }
  if (i >= a.n || !a.flag[i]) return;
  const uint64_t seq = a.next_seq + a.rank[i];
  a.table[a.slot_of[i]].seq = seq;
  // The ring slot belongs to the newest trace that maps to it.  An add that
  // creates more than ring_n traces (totals[0] of them) has several creators
  // per slot, and two 8-byte stores from unordered lanes: only the last of
  // them writes (the others' traces are evicted by it anyway), so the rebuild
  // re-inserts the live traces under their own ids.  With W > 1 ring_n is
  // pool_cap and created <= n <= pool_cap: every creator writes.
  if ((uint64_t)a.rank[i] + a.ring_n < a.totals[0]) return;
  const uint64_t r = seq % a.ring_n;
  a.ring_tid[2 * r] = a.cols.trace_id[2 * i];
  a.ring_tid[2 * r + 1] = a.cols.trace_id[2 * i + 1];
}

// the spans into the pool ring
template <bool kSql, bool kOtlp>
__global__ __launch_bounds__(kGbtThreads) void gbt_append_kernel(GbtArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (i >= a.n || gbt_batch_refused<kOtlp>(a)) return;
  const GbtPool& P = a.pool;
  const ose_columns& c = a.cols;
  const uint64_t p = (a.pool_pos + i) % a.pool_cap;
  const uint64_t h = a.slot_of[i];
  P.seq[p] = h == ~0ull ? kUnset : a.table[h].seq;
  P.tid[2 * p] = c.trace_id[2 * i];
  P.tid[2 * p + 1] = c.trace_id[2 * i + 1];
  P.start[p] = c.start_ns[i];
  P.end[p] = c.end_ns[i];
  P.status[p] = c.status[i];
  P.kind[p] = c.kind[i];
  P.url_flags[p] = c.url_flags ? c.url_flags[i] : 0;
  P.span_size[p] = c.span_size ? c.span_size[i] : 0;
  P.name_len[p] = c.name_len ? c.name_len[i] : 0;
  for (uint32_t w = 0; w < a.attr_words; w++)
    P.attr_match[w * a.pool_cap + p] = c.attr_match ? c.attr_match[w * a.n + i] : 0;
  P.origin[p] = a.scope_pos + c.scope[i];
  if constexpr (kSql) P.db_flags[p] = c.db_flags ? c.db_flags[i] : 0;
}

__device__ __forceinline__ void ring_copy(uint8_t* ring, uint64_t cap, uint64_t dst, const uint8_t* src, uint32_t n) {
  uint64_t q = dst % cap;
  for (uint32_t b = 0; b < n; b++) {
    ring[q] = src[b];
    if (++q == cap) q = 0;
  }
}

// ---- wave copies (the SQL instances) ----------------------------------------
//
// One wave takes 64 consecutive spans.  Each lane loads its own span's source,
// destination and length; the wave then walks the spans that have bytes (a
// ballot, the owner's values broadcast with v_readlane) and all 64 lanes move
// that span's bytes, consecutive lanes at consecutive addresses.  No LDS, no
// atomics, no waiting: every loop runs to a count read once.

__device__ __forceinline__ uint32_t wave_get(uint32_t v, uint32_t owner) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)owner);
}
__device__ __forceinline__ uint64_t wave_get(uint64_t v, uint32_t owner) {
  return (uint64_t)wave_get((uint32_t)(v >> 32), owner) << 32 | wave_get((uint32_t)v, owner);
}

// n bytes src -> dst by the whole wave, neither range wrapping.  Bytes up to
// the destination's first dword boundary, then one aligned dword store per
// lane fed by a dword load at the source's own alignment (gfx950 takes a
// misaligned global load; every byte read is inside [src, src + n)), then
// the bytes left after the last whole dword.  Right at every src and dst
// alignment.
__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane) {
  const uint32_t head = min(n, (uint32_t)(-(uintptr_t)dst & 3u));
  const uint32_t words = (n - head) >> 2, tail = (n - head) & 3u;
  if (lane < head) dst[lane] = src[lane];
  uint32_t* d = reinterpret_cast<uint32_t*>(dst + head);
  const uint8_t* s = src + head;
  for (uint32_t k = lane; k < words; k += 64) {
    uint32_t w;
    __builtin_memcpy(&w, s + 4ull * k, 4);
    d[k] = w;
  }
  const uint32_t t0 = head + 4 * words;
  if (lane < tail) dst[t0 + lane] = src[t0 + lane];
}

// The OTLP instances' move: messages are a few hundred bytes, so the middle
// goes as aligned 16-byte stores (one per lane, 1 KiB per wave step) fed by
// 16-byte loads at the source's own alignment; up to 15 bytes before the
// destination's first 16-byte boundary and after the last whole 16 go a byte
// per lane.  Every byte read is inside [src, src + n).
__device__ __forceinline__ void wave_copy16(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane) {
  const uint32_t head = min(n, (uint32_t)(-(uintptr_t)dst & 15u));
  const uint32_t quads = (n - head) >> 4, tail = (n - head) & 15u;
  if (lane < head) dst[lane] = src[lane];
  uint4* d = reinterpret_cast<uint4*>(dst + head);
  const uint8_t* s = src + head;
  for (uint32_t k = lane; k < quads; k += 64) {
    uint4 w;
    __builtin_memcpy(&w, s + 16ull * k, 16);
    d[k] = w;
  }
  const uint32_t t0 = head + 16 * quads;
  if (lane < tail) dst[t0 + lane] = src[t0 + lane];
}

// linear src -> the arena ring at position q < arena_cap, wrapping at its end
template <bool kWide = false>
__device__ __forceinline__ void wave_copy_in(const GbtArgs& a, uint64_t q, const uint8_t* src, uint32_t n, uint32_t lane) {
  const uint32_t first = (uint32_t)min<uint64_t>(n, a.arena_cap - q);
  if constexpr (kWide) {
    wave_copy16(a.arena_ring + q, src, first, lane);
    if (first < n) wave_copy16(a.arena_ring, src + first, n - first, lane);
  } else {
    wave_copy(a.arena_ring + q, src, first, lane);
    if (first < n) wave_copy(a.arena_ring, src + first, n - first, lane);
  }
}

// the arena ring from position q < arena_cap, read across its end -> linear dst
template <bool kWide = false>
__device__ __forceinline__ void wave_copy_out(const GbtArgs& a, uint8_t* dst, uint64_t q, uint32_t n, uint32_t lane) {
  const uint32_t first = (uint32_t)min<uint64_t>(n, a.arena_cap - q);
  if constexpr (kWide) {
    wave_copy16(dst, a.arena_ring + q, first, lane);
    if (first < n) wave_copy16(dst + first, a.arena_ring, n - first, lane);
  } else {
    wave_copy(dst, a.arena_ring + q, first, lane);
    if (first < n) wave_copy(dst + first, a.arena_ring, n - first, lane);
  }
}

// add: the batch's queries into the ring.  A span's query ends its block, so
// it lies at block + strlen - len (gbt_strings_kernel stores the same ref).
template <bool kOtlp>
__global__ __launch_bounds__(kGbtThreads) void gbt_query_copy_kernel(GbtArgs a) {
  if (gbt_batch_refused<kOtlp>(a)) return;
  const uint64_t i = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t len = 0, off = 0;
  uint64_t q = 0;
  if (i < a.n) {
    const ose_strref x = gbt_batch_query(a.cols, i);
    off = x.off;
    len = x.len;
    q = (a.arena_pos + a.stroff[i] + a.strlen[i] - len) % a.arena_cap;
  }
  for (uint64_t todo = __ballot(len != 0); todo; todo &= todo - 1) {
    const uint32_t o = (uint32_t)__builtin_ctzll(todo);
    wave_copy_in(a, wave_get(q, o), a.cols.arena + wave_get(off, o), wave_get(len, o), lane);
  }
}

// release: the released spans' blocks (route, path, attribute strings, query)
// out of the ring; consecutive spans' blocks are consecutive in the released
// arena.  gbt_emit_kernel<true> writes the refs and leaves the bytes to this.
// OTLP mode: the block starts with the span's message, and a fragment's
// first span has the fragment's header block moved ahead of its own.
template <bool kOtlp>
__global__ __launch_bounds__(kGbtThreads) void gbt_block_copy_kernel(GbtArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t len = 0, base = 0, hlen = 0;
  uint64_t q = 0, hq = 0;
  if (j < a.n) {
    len = a.strlen[j];
    base = a.stroff[j];
    const uint64_t p = (a.pool_pos + a.order[j]) % a.pool_cap;
    q = a.pool.str_off[p] % a.arena_cap;
    if constexpr (kOtlp) {
      if (a.flag[j]) {
        const uint64_t o = a.pool.origin[p] % a.scope_cap;
        hlen = a.otlp.hdr_res[o] + a.otlp.hdr_scope[o];
        hq = a.otlp.hdr_off[o] % a.arena_cap;
        len -= hlen;   // gbt_gather_kernel counted the header with the span
      }
    }
  }
  if constexpr (kOtlp) {
    for (uint64_t todo = __ballot(hlen != 0); todo; todo &= todo - 1) {
      const uint32_t o = (uint32_t)__builtin_ctzll(todo);
      wave_copy_out<true>(a, a.out.arena + wave_get(base, o), wave_get(hq, o), wave_get(hlen, o), lane);
    }
    base += hlen;
  }
  for (uint64_t todo = __ballot(len != 0); todo; todo &= todo - 1) {
    const uint32_t o = (uint32_t)__builtin_ctzll(todo);
    wave_copy_out<kOtlp>(a, a.out.arena + wave_get(base, o), wave_get(q, o), wave_get(len, o), lane);
  }
}

// ---- OTLP mode: messages and header blocks -----------------------------------

// add: the batch's Span messages to the head of their blocks, a wave per 64
// consecutive spans and all 64 lanes on one message (as gbt_query_copy_kernel)
__global__ __launch_bounds__(kGbtThreads) void gbt_msg_copy_kernel(GbtArgs a) {
  if (gbt_batch_refused<true>(a)) return;
  const uint64_t i = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t len = 0, off = 0;
  uint64_t q = 0;
  if (i < a.n) {
    const uint64_t ref = a.otlp.span_ref[i];
    off = (uint32_t)ref;
    len = (uint32_t)(ref >> 32);
    q = (a.arena_pos + a.stroff[i]) % a.arena_cap;
  }
  for (uint64_t todo = __ballot(len != 0); todo; todo &= todo - 1) {
    const uint32_t o = (uint32_t)__builtin_ctzll(todo);
    wave_copy_in<true>(a, wave_get(q, o), a.cols.arena + wave_get(off, o), wave_get(len, o), lane);
  }
}

// The top-level fields of the payload [s, e) other than the LEN field `drop`
// (ResourceSpans.scope_spans, ScopeSpans.spans: both field 2): their bytes,
// and with kCopy each field as it stands into the ring from position *dst on.
// false: malformed (the decoder walked these payloads, so a bug).
template <bool kCopy>
__device__ bool gbt_hdr_fields(const GbtArgs& a, uint32_t s, uint32_t e, uint32_t* bytes, uint64_t* dst) {
  pbdev::Rd r(a.cols.arena, s, e);
  uint32_t total = 0;
  while (r.more()) {
    const uint32_t f0 = r.i;
    uint32_t f, wt;
    if (!r.tag(f, wt) || !r.skip(wt)) break;
    if (f == 2 && wt == 2) continue;
    const uint32_t n = r.i - f0;
    if constexpr (kCopy) {
      uint64_t q = *dst % a.arena_cap;
      for (uint32_t b = 0; b < n; b++) {
        a.arena_ring[q] = a.cols.arena[f0 + b];
        if (++q == a.arena_cap) q = 0;
      }
      *dst += n;
    }
    total += n;
  }
  *bytes = total;
  return !r.bad;
}

// add: every added scope's header lengths, one lane per scope
__global__ __launch_bounds__(kGbtThreads) void gbt_hdr_len_kernel(GbtArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (s >= a.n_scopes) return;
  const uint64_t rr = a.otlp.res_ref[a.cols.scope_resource[s]], sr = a.otlp.scope_ref[s];
  uint32_t hr = 0, hs = 0;
  const bool ok = gbt_hdr_fields<false>(a, (uint32_t)rr, (uint32_t)rr + (uint32_t)(rr >> 32), &hr, nullptr) &&
                  gbt_hdr_fields<false>(a, (uint32_t)sr, (uint32_t)sr + (uint32_t)(sr >> 32), &hs, nullptr);
  if (!ok) {
    atomicOr(a.error, kGbtErrHeader);
    hr = hs = 0;
  }
  a.otlp.hres[s] = hr;
  a.otlp.hscope[s] = hs;
  a.otlp.hlen[s] = hr + hs;
}

// ... and their bytes into the ring, after the call's span blocks
__global__ __launch_bounds__(kGbtThreads) void gbt_hdr_copy_kernel(GbtArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (s >= a.n_scopes || gbt_batch_refused<true>(a) || !a.otlp.hlen[s]) return;
  const uint64_t rr = a.otlp.res_ref[a.cols.scope_resource[s]], sr = a.otlp.scope_ref[s];
  uint64_t dst = a.arena_pos + a.totals[1] + a.otlp.hoff[s];
  uint32_t n;
  gbt_hdr_fields<true>(a, (uint32_t)rr, (uint32_t)rr + (uint32_t)(rr >> 32), &n, &dst);
  gbt_hdr_fields<true>(a, (uint32_t)sr, (uint32_t)sr + (uint32_t)(sr >> 32), &n, &dst);
}

// The bytes of the call in 64 bits: strlen[0, n) and, on the add, hlen[0,
// n_scopes).  The u32 scans give the offsets; this total decides the refusal
// and sizes the release, so a wrapped scan total is never acted on.  One
// atomic per wave.
__global__ __launch_bounds__(kGbtThreads) void gbt_total_kernel(GbtArgs a) {
  uint64_t sum = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kGbtThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x; i < a.n; i += stride) sum += a.strlen[i];
  for (uint64_t s = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x; s < a.n_scopes; s += stride) sum += a.otlp.hlen[s];
  for (int d = 32; d; d >>= 1) sum += __shfl_down(sum, d, 64);
  if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(reinterpret_cast<unsigned long long*>(a.otlp.total64), (unsigned long long)sum);
}

// release: each fragment's InstrumentationScope and schema_url refs from its
// moved ScopeSpans part, by the decoder's rule (otlp_scope_count_kernel): the
// scope field, kOtlpScopeMulti when several, the last schema_url
__global__ __launch_bounds__(kGbtThreads) void gbt_frag_hdr_kernel(GbtArgs a, uint64_t n_frag) {
  const uint64_t f = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (f >= n_frag) return;
  const uint64_t ref = a.otlp.out_scope_ref[f];
  pbdev::Rd r(a.out.arena, (uint32_t)ref, (uint32_t)ref + (uint32_t)(ref >> 32));
  uint64_t hdr = 0, schema = 0;
  uint32_t nh = 0, fld, wt;
  while (r.more() && r.tag(fld, wt)) {
    uint32_t ps, pl;
    if (fld == 1 || fld == 3) {
      if (wt != 2 || !r.len(ps, pl)) { r.bad = true; break; }
      if (fld == 1) { hdr = (uint64_t)ps | ((uint64_t)pl << 32); nh++; }
      else schema = (uint64_t)ps | ((uint64_t)pl << 32);
    } else {
      r.skip(wt);
    }
  }
  if (r.bad) atomicOr(a.error, kGbtErrHeader);
  a.otlp.out_hdr[f] = nh > 1 ? kOtlpScopeMulti : hdr;
  a.otlp.out_schema[f] = schema;
}

// the string block: route, path, then the string attribute values (kSql: then
// the query); refs in the pool are relative to the block
template <bool kSql, bool kOtlp>
__global__ __launch_bounds__(kGbtThreads) void gbt_strings_kernel(GbtArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (i >= a.n || gbt_batch_refused<kOtlp>(a)) return;
  const GbtPool& P = a.pool;
  const ose_columns& c = a.cols;
  const uint64_t p = (a.pool_pos + i) % a.pool_cap;
  const uint64_t blk = a.arena_pos + a.stroff[i];
  P.str_off[p] = blk;
  uint32_t rel = 0;
  if constexpr (kOtlp) {   // the message first (gbt_msg_copy_kernel moves it): every ref below shifts by its length
    rel = (uint32_t)(a.otlp.span_ref[i] >> 32);
    a.otlp.msg_len[p] = rel;
  }
  ose_strref r{0, 0};
  if (c.route) {
    const ose_strref x = c.route[i];
    ring_copy(a.arena_ring, a.arena_cap, blk + rel, c.arena + x.off, x.len);
    r = ose_strref{rel, x.len};
    rel += x.len;
  }
  P.route[p] = r;
  r = ose_strref{0, 0};
  if (c.path) {
    const ose_strref x = c.path[i];
    ring_copy(a.arena_ring, a.arena_cap, blk + rel, c.arena + x.off, x.len);
    r = ose_strref{rel, x.len};
    rel += x.len;
  }
  P.path[p] = r;
  for (uint32_t k = 0; k < a.n_attr_keys; k++) {
    const uint8_t t = c.attr_type[(uint64_t)k * a.n + i];
    uint64_t v = c.attr_val[(uint64_t)k * a.n + i];
    if (t == OSE_ATTR_STR) {
      const uint32_t off = (uint32_t)v, len = (uint32_t)(v >> 32);
      ring_copy(a.arena_ring, a.arena_cap, blk + rel, c.arena + off, len);
      v = (uint64_t)rel | ((uint64_t)len << 32);
      rel += len;
    }
    P.attr_type[(uint64_t)k * a.pool_cap + p] = t;
    P.attr_val[(uint64_t)k * a.pool_cap + p] = v;
  }
  if constexpr (kSql) {
    const ose_strref x = gbt_batch_query(c, i);
    const bool has = c.db_flags && (c.db_flags[i] & OSE_DB_HAS_QUERY);
    if (!kWaveCopy) ring_copy(a.arena_ring, a.arena_cap, blk + rel, c.arena + x.off, x.len);   // else gbt_query_copy_kernel
    P.db_query[p] = has ? ose_strref{rel, x.len} : ose_strref{0, 0};
  }
}

// the batch's scopes into the scope ring, with their resource's columns
template <bool kSql, bool kOtlp>
__global__ __launch_bounds__(kGbtThreads) void gbt_scopes_kernel(GbtArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (s >= a.n_scopes || gbt_batch_refused<kOtlp>(a)) return;
  const ose_columns& c = a.cols;
  const GbtScopes& Q = a.scopes;
  const uint64_t q = (a.scope_pos + s) % a.scope_cap;
  const uint32_t r = c.scope_resource[s];
  Q.res_svc[q] = c.res_svc[r];
  Q.res_svc_str[q] = c.res_svc_str ? c.res_svc_str[r] : c.res_svc[r];
  Q.res_url_ok[q] = c.res_url_ok ? c.res_url_ok[r] : 1;
  const uint32_t set = c.res_attrset[r];
  Q.res_attrset[q] = a.attrset_map ? a.attrset_map[set] : set;
  Q.res_size[q] = c.res_size ? c.res_size[r] : 0;
  Q.scope_size[q] = c.scope_size ? c.scope_size[s] : 0;
  if constexpr (kSql) Q.res_sql_ok[q] = c.res_sql_ok ? c.res_sql_ok[r] : 1;   // NULL: every resource passes
  if constexpr (kOtlp) {   // the header blocks follow the call's span blocks (totals[1] bytes: not refused, so no wrap)
    a.otlp.hdr_off[q] = a.arena_pos + a.totals[1] + a.otlp.hoff[s];
    a.otlp.hdr_res[q] = a.otlp.hres[s];
    a.otlp.hdr_scope[q] = a.otlp.hscope[s];
  }
}

// ---- per-worker numbering (num_workers > 1), after the add's kernels -------

// the batch's new traces as (worker, creation rank) pairs, and how many each
// worker gets
__global__ __launch_bounds__(kGbtThreads) void gbt_wkey_kernel(GbtArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (i >= a.n || !a.flag[i]) return;
  const uint32_t k = a.rank[i];
  const uint32_t w = gbt_worker(a.cols.trace_id[2 * i], a.cols.trace_id[2 * i + 1], a.n_workers);
  a.keys[k] = w;
  a.vals[k] = k;
  atomicAdd(&a.wadd[w], 1u);
}

// the pairs stably sorted by worker: the j-th is its worker's
// (j - wstart[w])-th new trace, after the wcnt[w] it had
__global__ __launch_bounds__(kGbtThreads) void gbt_wnum_kernel(GbtArgs a, uint64_t created) {
  const uint64_t j = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (j >= created) return;
  const uint32_t w = a.keys[j];
  const uint64_t q = a.wcnt[w] + (j - a.wstart[w]);
  a.tinfo[(a.next_seq + a.vals[j]) % a.ring_n] = (uint64_t)w << 40 | q;
}

// ---- release ---------------------------------------------------------------

// the pool window's spans of released traces (seq in [rel_lo, rel_hi))
__global__ __launch_bounds__(kGbtThreads) void gbt_flag_kernel(GbtArgs a) {
  const uint64_t w = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (w >= a.n) return;
  const uint64_t seq = a.pool.seq[(a.pool_pos + w) % a.pool_cap];
  a.flag[w] = seq >= a.rel_lo && seq < a.rel_hi && !gbt_evicted(a, seq);
}

__global__ __launch_bounds__(kGbtThreads) void gbt_compact_kernel(GbtArgs a) {
  const uint64_t w = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (w >= a.n || !a.flag[w]) return;
  const uint32_t d = a.rank[w];
  a.keys[d] = (uint32_t)(a.pool.seq[(a.pool_pos + w) % a.pool_cap] - a.rel_lo);
  a.vals[d] = (uint32_t)w;
}

// output span j <- pool window position order[j]: fixed columns, fragment
// heads (a new trace or a new origin scope), string block lengths
template <bool kSql, bool kOtlp>
__global__ __launch_bounds__(kGbtThreads) void gbt_gather_kernel(GbtArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (j >= a.n) return;
  const GbtPool& P = a.pool;
  const GbtOut& O = a.out;
  const uint64_t p = (a.pool_pos + a.order[j]) % a.pool_cap;
  O.tid[2 * j] = P.tid[2 * p];
  O.tid[2 * j + 1] = P.tid[2 * p + 1];
  O.start[j] = P.start[p];
  O.end[j] = P.end[p];
  O.status[j] = P.status[p];
  O.kind[j] = P.kind[p];
  O.url_flags[j] = P.url_flags[p];
  O.span_size[j] = P.span_size[p];
  O.name_len[j] = P.name_len[p];
  for (uint32_t w = 0; w < a.attr_words; w++) O.attr_match[w * a.n + j] = P.attr_match[w * a.pool_cap + p];
  uint32_t head = 1;
  if (j > 0) {
    const uint64_t q = (a.pool_pos + a.order[j - 1]) % a.pool_cap;
    head = P.seq[q] != P.seq[p] || P.origin[q] != P.origin[p];
  }
  a.flag[j] = head;
  uint32_t len = P.route[p].len + P.path[p].len;
  for (uint32_t k = 0; k < a.n_attr_keys; k++)
    if (P.attr_type[(uint64_t)k * a.pool_cap + p] == OSE_ATTR_STR)
      len += (uint32_t)(P.attr_val[(uint64_t)k * a.pool_cap + p] >> 32);
  if constexpr (kSql) {
    O.db_flags[j] = P.db_flags[p];
    len += P.db_query[p].len;
  }
  if constexpr (kOtlp) {   // the message, and ahead of a fragment's first span its header block
    len += a.otlp.msg_len[p];
    if (head) {
      const uint64_t o = P.origin[p] % a.scope_cap;
      len += a.otlp.hdr_res[o] + a.otlp.hdr_scope[o];
    }
  }
  a.strlen[j] = len;
}

// strings, refs, resource / scope ids and the fragment columns
template <bool kSql, bool kOtlp>
__global__ __launch_bounds__(kGbtThreads) void gbt_emit_kernel(GbtArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * kGbtThreads + threadIdx.x;
  if (j >= a.n) return;
  const GbtPool& P = a.pool;
  const GbtOut& O = a.out;
  const uint64_t p = (a.pool_pos + a.order[j]) % a.pool_cap;
  const uint32_t f = a.rank[j] + a.flag[j] - 1;   // fragment index (inclusive scan - 1)
  O.resource[j] = f;
  O.scope[j] = f;
  uint32_t base = a.stroff[j];
  if constexpr (kOtlp) {
    if (a.flag[j]) {   // the fragment's header block, then this span's block
      const uint64_t o = P.origin[p] % a.scope_cap;
      const uint32_t hr = a.otlp.hdr_res[o], hs = a.otlp.hdr_scope[o];
      a.otlp.out_res_ref[f] = (uint64_t)base | (uint64_t)hr << 32;
      a.otlp.out_scope_ref[f] = (uint64_t)(base + hr) | (uint64_t)hs << 32;
      a.otlp.out_span0[f] = (uint32_t)j;
      a.otlp.out_res_scope0[f] = f;
      base += hr + hs;
    }
    a.otlp.out_span_ref[j] = (uint64_t)base | (uint64_t)a.otlp.msg_len[p] << 32;
  }
  const uint64_t blk = P.str_off[p];
  const uint32_t len = P.route[p].len + P.path[p].len;
  uint32_t total = len;
  for (uint32_t k = 0; k < a.n_attr_keys; k++)
    if (P.attr_type[(uint64_t)k * a.pool_cap + p] == OSE_ATTR_STR)
      total += (uint32_t)(P.attr_val[(uint64_t)k * a.pool_cap + p] >> 32);
  if constexpr (kSql) {
    const ose_strref x = P.db_query[p];
    const bool has = P.db_flags[p] & OSE_DB_HAS_QUERY;
    O.db_query[j] = has ? ose_strref{base + x.off, x.len} : ose_strref{0, 0};
    total += x.len;
  }
  if (!kOtlp && (!kSql || !kWaveCopy)) {   // else gbt_block_copy_kernel moves the block
    uint64_t q0 = blk % a.arena_cap;
    for (uint32_t b = 0; b < total; b++) {
      O.arena[base + b] = a.arena_ring[q0];
      if (++q0 == a.arena_cap) q0 = 0;
    }
  }
  const ose_strref r = P.route[p], q = P.path[p];
  O.route[j] = ose_strref{base + r.off, r.len};
  O.path[j] = ose_strref{base + q.off, q.len};
  for (uint32_t k = 0; k < a.n_attr_keys; k++) {
    const uint8_t t = P.attr_type[(uint64_t)k * a.pool_cap + p];
    uint64_t v = P.attr_val[(uint64_t)k * a.pool_cap + p];
    if (t == OSE_ATTR_STR) v = (uint64_t)(base + (uint32_t)v) | (v & 0xFFFFFFFF00000000ull);
    O.attr_type[(uint64_t)k * a.n + j] = t;
    O.attr_val[(uint64_t)k * a.n + j] = v;
  }
  if (a.flag[j]) {
    const GbtScopes& Q = a.scopes;
    const uint64_t o = P.origin[p] % a.scope_cap;
    O.res_svc[f] = Q.res_svc[o];
    O.res_svc_str[f] = Q.res_svc_str[o];
    O.res_url_ok[f] = Q.res_url_ok[o];
    O.res_attrset[f] = Q.res_attrset[o];
    O.res_size[f] = Q.res_size[o];
    O.scope_size[f] = Q.scope_size[o];
    O.scope_resource[f] = f;
    if constexpr (kSql) O.res_sql_ok[f] = Q.res_sql_ok[o];
  }
}

uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kGbtThreads - 1) / kGbtThreads); }
}  // namespace

#define GBT_LAUNCH(k, n) hipLaunchKernelGGL(k, dim3(blocks_for(n)), dim3(kGbtThreads), 0, st, a)

void launch_gbt_rebuild(const GbtArgs& a, hipStream_t st) {
  const uint64_t n = a.live_hi - a.live_lo;
  if (!n) return;
  const uint32_t b = (uint32_t)std::min<uint64_t>(blocks_for(n), 4096);
  hipLaunchKernelGGL(gbt_rebuild_kernel, dim3(b), dim3(kGbtThreads), 0, st, a);
}
void launch_gbt_lookup(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH(gbt_lookup_kernel, a.n); }
// the SQL instance on a store that carries the three columns, else the plain
// one; the OTLP instance on a store fed by ose_gbt_add_otlp
#define GBT_LAUNCH_MODE(k, n)                                                                 \
  do {                                                                                        \
    void (*fn)(GbtArgs) = a.otlp.on ? (a.sql ? k<true, true> : k<false, true>)                \
                                    : (a.sql ? k<true, false> : k<false, false>);             \
    hipLaunchKernelGGL(fn, dim3(blocks_for(n)), dim3(kGbtThreads), 0, st, a);                 \
  } while (0)
#define GBT_LAUNCH_OTLP(k, n)                                                                 \
  do {                                                                                        \
    void (*fn)(GbtArgs) = a.otlp.on ? k<true> : k<false>;                                     \
    hipLaunchKernelGGL(fn, dim3(blocks_for(n)), dim3(kGbtThreads), 0, st, a);                 \
  } while (0)
void launch_gbt_creator(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH_MODE(gbt_creator_kernel, a.n); }
void launch_gbt_assign(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH_OTLP(gbt_assign_kernel, a.n); }
void launch_gbt_append(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH_MODE(gbt_append_kernel, a.n); }
void launch_gbt_strings(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH_MODE(gbt_strings_kernel, a.n); }
void launch_gbt_scopes(const GbtArgs& a, hipStream_t st) {
  if (a.n_scopes) GBT_LAUNCH_MODE(gbt_scopes_kernel, a.n_scopes);
}
void launch_gbt_flag(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH(gbt_flag_kernel, a.n); }
void launch_gbt_compact(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH(gbt_compact_kernel, a.n); }
void launch_gbt_gather(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH_MODE(gbt_gather_kernel, a.n); }
void launch_gbt_emit(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH_MODE(gbt_emit_kernel, a.n); }
void launch_gbt_query_copy(const GbtArgs& a, hipStream_t st) {
  if (a.sql && kWaveCopy && a.cols.db_flags) GBT_LAUNCH_OTLP(gbt_query_copy_kernel, a.n);
}
void launch_gbt_block_copy(const GbtArgs& a, hipStream_t st) {
  if (a.otlp.on || (a.sql && kWaveCopy)) GBT_LAUNCH_OTLP(gbt_block_copy_kernel, a.n);
}
void launch_gbt_hdr_len(const GbtArgs& a, hipStream_t st) {
  if (a.n_scopes) GBT_LAUNCH(gbt_hdr_len_kernel, a.n_scopes);
}
void launch_gbt_total(const GbtArgs& a, hipStream_t st) {
  const uint64_t n = std::max(a.n, a.n_scopes);
  if (n) hipLaunchKernelGGL(gbt_total_kernel, dim3(std::min<uint32_t>(blocks_for(n), 1024)), dim3(kGbtThreads), 0, st, a);
}
void launch_gbt_msg_copy(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH(gbt_msg_copy_kernel, a.n); }
void launch_gbt_hdr_copy(const GbtArgs& a, hipStream_t st) {
  if (a.n_scopes) GBT_LAUNCH(gbt_hdr_copy_kernel, a.n_scopes);
}
void launch_gbt_frag_hdr(const GbtArgs& a, uint64_t n_frag, hipStream_t st) {
  if (n_frag) hipLaunchKernelGGL(gbt_frag_hdr_kernel, dim3(blocks_for(n_frag)), dim3(kGbtThreads), 0, st, a, n_frag);
}
void launch_gbt_wkey(const GbtArgs& a, hipStream_t st) { GBT_LAUNCH(gbt_wkey_kernel, a.n); }
void launch_gbt_wnum(const GbtArgs& a, uint64_t created, hipStream_t st) {
  if (created) hipLaunchKernelGGL(gbt_wnum_kernel, dim3(blocks_for(created)), dim3(kGbtThreads), 0, st, a, created);
}

}  // namespace ose
