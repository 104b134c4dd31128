// gbt_host.cpp — the GPU-resident groupbytrace store:
// ose_gbt_*.  Restates groupbytraceprocessor (opentelemetry-collector-contrib
// v0.141.0, `collector/builder-config.yaml:73`; not in the reference tree)
// as Odigos configures it (`autoscaler/controllers/actions/sampling/
// groupbytrace.go:3-9`: wait_duration "30s"; num_traces and num_workers at
// their defaults, 1,000,000 and 1; other num_workers are taken too):
//   * ConsumeTraces splits the batch per (ResourceSpans, ScopeSpans, trace
//     id) (batchpersignal.SplitTraces) and hands each piece to the event
//     machine in that order;
//   * the first piece of an unknown trace id puts it in the ring buffer of
//     num_traces ids — evicting (dropping) the trace that slot held — and
//     arms a timer of wait_duration; later pieces append to the trace;
//   * on expiry the trace leaves the buffer and goes downstream as one
//     ptrace.Traces holding its pieces in arrival order; spans of that id
//     arriving afterwards start a new trace;
//   * num_workers W > 1: the event machine hands a trace's events to worker
//     fnv64(id) % W, each worker with a ring of num_traces / W ids, so a
//     trace is evicted by the (num_traces / W)-th trace created after it in
//     its own worker.
// Time is the caller's clock (now_ns on every call), so releases are
// deterministic.  The kernels are in gbt_kernel.hip, the scratch layouts and
// the control words in gbt_layout.hpp.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "engine_internal.hpp"
#include "gbt_layout.hpp"
#include "kernels.hpp"
#include "slab.hpp"

namespace ose {

namespace {
struct DevMem {   // grow-only device buffer
  uint8_t* p = nullptr;
  size_t cap = 0;
  int need(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = up(std::max<size_t>(bytes + bytes / 4, 1 << 16), 1 << 16);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), want));
    cap = want;
    return 0;
  }
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
};
template <class T>
T* part_ptr(const DevMem& b, const WsPart& p) { return reinterpret_cast<T*>(b.p + p.off); }

// Go's time.ParseDuration: [-+]?([0-9]*(\.[0-9]*)?unit)+ or "0"
bool parse_go_duration(const std::string& s, int64_t& out) {
  size_t i = 0;
  bool neg = false;
  if (i < s.size() && (s[i] == '-' || s[i] == '+')) neg = s[i++] == '-';
  if (s.substr(i) == "0") { out = 0; return true; }
  if (i == s.size()) return false;
  double total = 0;
  while (i < s.size()) {
    const size_t d0 = i;
    uint64_t v = 0;
    while (i < s.size() && s[i] >= '0' && s[i] <= '9') v = v * 10 + (uint64_t)(s[i++] - '0');
    double frac = 0, scale = 1;
    const bool int_digits = i > d0;
    bool frac_digits = false;
    if (i < s.size() && s[i] == '.') {
      i++;
      while (i < s.size() && s[i] >= '0' && s[i] <= '9') {
        frac = frac * 10 + (s[i++] - '0');
        scale *= 10;
        frac_digits = true;
      }
    }
    if (!int_digits && !frac_digits) return false;
    const size_t u0 = i;
    while (i < s.size() && !(s[i] >= '0' && s[i] <= '9') && s[i] != '.') i++;
    const std::string unit = s.substr(u0, i - u0);
    double mult;
    if (unit == "ns") mult = 1;
    else if (unit == "us" || unit == "\xC2\xB5s" || unit == "\xCE\xBCs") mult = 1e3;
    else if (unit == "ms") mult = 1e6;
    else if (unit == "s") mult = 1e9;
    else if (unit == "m") mult = 60e9;
    else if (unit == "h") mult = 3600e9;
    else return false;
    total += (double)v * mult + frac / scale * mult;
  }
  if (total > 9.2e18) return false;
  out = (int64_t)std::llround(neg ? -total : total);
  return true;
}
}  // namespace

struct Gbt {
  Engine* e = nullptr;
  int64_t wait_ns = 0;
  uint64_t num_traces = 1000000;
  uint32_t W = 1;                 // num_workers
  uint64_t ring_n = 0, wcap = 0;  // ring slots (num_traces, or the pool capacity when W > 1); num_traces / W
  std::vector<uint64_t> wcnt;     // per worker: traces numbered
  std::vector<uint64_t> wrel;     // per worker: its traces with seq < rel_end (released or evicted)
  uint32_t K = 0;
  bool sql = false;               // the engine has the odigossqldboperationprocessor section: db_flags,
                                  // db_query and res_sql_ok are carried (else ignored, and released NULL)
  uint64_t pool_cap = 0, scope_cap = 0, arena_cap = 0;
  // device state
  DevMem table, ring, pool, scopes, arena, scratch, sortbuf, out, words, tinfo, wdev;
  // The first successful add fixes the mode: columns (ose_gbt_add) or OTLP
  // (ose_gbt_add_otlp: the blocks start with the Span message, every added
  // scope has a header block; omem holds the rings' extra columns and `rel`
  // is the batch ose_gbt_release_otlp hands out, owned here)
  enum Mode { kUnset, kColumns, kOtlp } mode = kUnset;
  DevMem omem;
  GbtOtlp O2{};
  ose_otlp_batch* rel = nullptr;
  // diagnostics (osehost_gbt_copy_times): HIP events around the two OTLP wave
  // copies, the message copy of the last add and the block copy of the last release
  bool time_copies = false;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  float copy_ms[2] = {0, 0};
  ~Gbt() {
    if (rel) otlp_released_delete(rel);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  uint64_t table_slots = 0;
  uint32_t epoch = 0;
  GbtPool P{};
  GbtScopes Q{};
  // host clock
  uint64_t next_seq = 0, rel_end = 0;
  uint64_t pool_begin = 0, pool_end = 0, scope_begin = 0, scope_end = 0, arena_begin = 0, arena_end = 0;
  struct Epoch {
    int64_t t;
    uint64_t seq1, pool1, scope1, arena1;
    std::vector<uint64_t> wcnt1;   // W > 1: the workers' counts after the call
  };
  std::deque<Epoch> epochs;
  uint32_t n_attrsets = 0;
  int64_t last_now = INT64_MIN;   // the clock of the last successful call
  // the last release
  ose_columns out_cols{};
  // stats: created, released traces, evicted traces, released spans, added spans
  uint64_t created = 0, released = 0, evicted = 0, released_spans = 0, added_spans = 0;

  // the persistent id table (gbt_kernel.hip): slots claimed since its last
  // rebuild (live ids and tombstones), the number of the last add
  uint64_t slots_used = 0;
  uint32_t add_gen = 0;
  bool table_valid = false;

  GbtWords* ctl() const { return reinterpret_cast<GbtWords*>(words.p); }   // the control words (device)
  // one worker: the traces a ring of num_traces has evicted (W > 1: per trace, gbt_evicted)
  uint64_t evict_below() const { return W == 1 && next_seq > num_traces ? next_seq - num_traces : 0; }
  // W > 1: worker w's traces [0, this) are evicted
  uint64_t w_evicted(uint32_t w) const { return wcnt[w] > wcap ? wcnt[w] - wcap : 0; }
  uint64_t waiting() const {
    if (W == 1) return next_seq - live_lo();
    uint64_t n = 0;
    for (uint32_t w = 0; w < W; w++) n += wcnt[w] - std::max(wrel[w], w_evicted(w));
    return n;
  }
  uint64_t live_lo() const { return std::max(rel_end, evict_below()); }
  // traces whose wait is over at `now`: [.., expired_below(now)) (created by
  // the calls at least wait_duration ago; the next release hands them out)
  uint64_t expired_below(int64_t now) const {
    uint64_t b = rel_end;
    for (const Epoch& ep : epochs) {
      if (ep.t + wait_ns > now) break;
      b = std::max(b, ep.seq1);
    }
    return b;
  }
};

namespace {
// Reserves the control words for scans of up to n items: the named words, the
// look-back status of that scan's tiles, and a fixed margin.  An entry point
// calls it once, before base_args hands pointers into the words to GbtArgs (a
// buffer that grew later would leave them dangling), with the most items any
// of its scans has.  That covers the sort's scan too: it runs over 256 * T
// counts for the T = ceil(m / kSortTile) tiles of m <= n pairs, which is
// ceil(m / 16384) scan tiles, never more than the ceil(n / 1024) of n items.
int words_need(Gbt* g, uint64_t n) {
  const uint64_t tiles = (n + kScanTileItems - 1) / kScanTileItems;
  return g->words.need(offsetof(GbtWords, status) + sizeof(uint64_t) * (tiles + 256 * 4 + 16));
}

// the first `bytes` of the control words (a kGbtWords* prefix) on the host, once the stream's work is done
int read_words(Gbt* g, GbtWords& h, size_t bytes, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(&h, g->words.p, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

// exclusive scan of n u32 (flags or lengths) with the shared look-back scan
int scan_u32(Gbt* g, const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* total, hipStream_t st) {
  if (!n) return 0;
  const uint32_t tiles = (uint32_t)((n + kScanTileItems - 1) / kScanTileItems);
  GbtWords* w = g->ctl();
  if (offsetof(GbtWords, status) + (uint64_t)tiles * 8 > g->words.cap)
    return fail(OSE_EDEVICE, "groupbytrace: scan status too small");
  HIP_TRY(hipMemsetAsync(&w->scan_counter, 0, 4, st));
  HIP_TRY(hipMemsetAsync(w->status, 0, (size_t)tiles * 8, st));
  ScanArgs sa{};
  sa.n = n;
  sa.n_tiles = tiles;
  sa.in = in;
  sa.out = out;
  sa.total = total;
  sa.counter = &w->scan_counter;
  sa.status = w->status;
  sa.error = &w->error;
  launch_scan_u32(sa, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

// stable LSD radix sort of m (key, value) pairs on the keys' low `bits` bits
// (the sampling stage's sort kernels: radix_passes); *skeys / *svals: the
// sorted arrays (the inputs when m <= 1 or bits == 0)
int sort_pairs(Gbt* g, const uint32_t* keys, const uint32_t* vals, uint64_t m, int bits, hipStream_t st,
               const uint32_t** skeys, const uint32_t** svals) {
  *skeys = keys;
  *svals = vals;
  if (m <= 1 || !bits) return 0;
  const uint32_t T = (uint32_t)((m + kSortTile - 1) / kSortTile);
  const uint32_t htiles = (uint32_t)((256ull * T + kScanTileItems - 1) / kScanTileItems);
  const GbtSortLayout L = gbt_sort_layout(m, T);
  if (int rc = g->sortbuf.need(L.end)) return rc;
  GbtWords* w = g->ctl();   // (its scan status: reserved by the entry point's words_need)
  HIP_TRY(hipMemsetAsync(&w->sort_gate, 1, 4, st));   // open
  TraceSortArgs s{};
  s.n_spans = m;
  s.n_tiles = T;
  s.gate = &w->sort_gate;
  s.error = &w->error;
  s.key = const_cast<uint32_t*>(keys);
  s.scan_counter = &w->scan_counter;
  s.scan_status = w->status;
  uint32_t* const kb[2] = {part_ptr<uint32_t>(g->sortbuf, L.k2), part_ptr<uint32_t>(g->sortbuf, L.k3)};
  uint32_t* const vb[2] = {part_ptr<uint32_t>(g->sortbuf, L.v2), part_ptr<uint32_t>(g->sortbuf, L.v3)};
  return radix_passes(s, kb, vb, part_ptr<uint32_t>(g->sortbuf, L.hist), part_ptr<uint32_t>(g->sortbuf, L.hoff), htiles,
                      bits, keys, vals, st, skeys, svals);
}

GbtArgs base_args(Gbt* g) {
  GbtArgs a{};
  a.table = reinterpret_cast<GbtSlot*>(g->table.p);
  a.table_mask = g->table_slots - 1;
  a.epoch = g->epoch;
  a.n_attr_keys = g->K;
  a.attr_words = g->e->attr_words;
  a.error = &g->ctl()->error;
  a.ring_tid = reinterpret_cast<uint64_t*>(g->ring.p);
  a.num_traces = g->num_traces;
  a.ring_n = g->ring_n;
  a.n_workers = g->W;
  a.worker_cap = g->wcap;
  if (g->W > 1) {
    const GbtWorkerLayout L = gbt_worker_layout(g->W);
    a.tinfo = reinterpret_cast<uint64_t*>(g->tinfo.p);
    a.wcnt = part_ptr<const uint64_t>(g->wdev, L.wcnt);
    a.wadd = part_ptr<uint32_t>(g->wdev, L.wadd);
    a.wstart = part_ptr<uint32_t>(g->wdev, L.wstart);
  }
  a.pool = g->P;
  a.pool_cap = g->pool_cap;
  a.scopes = g->Q;
  a.scope_cap = g->scope_cap;
  a.arena_ring = g->arena.p;
  a.arena_cap = g->arena_cap;
  a.sql = g->sql;
  if (g->mode == Gbt::kOtlp) {
    a.otlp = g->O2;
    a.otlp.on = 1;
    a.otlp.total64 = &g->ctl()->total64;
  }
  return a;
}

// W > 1: the workers' counts as the call finds them (its lookups, the rebuild
// and the release flags skip evicted traces)
int upload_worker_counts(Gbt* g, hipStream_t st) {
  uint8_t* wcnt = g->wdev.p + gbt_worker_layout(g->W).wcnt.off;
  HIP_TRY(hipMemcpyAsync(wcnt, g->wcnt.data(), 8ull * g->W, hipMemcpyHostToDevice, st));
  return 0;
}

// num_workers > 1: each new trace of the add gets its worker and its number
// within the worker (creation order), kept in tinfo; the workers' counts grow
int number_workers(Gbt* g, GbtArgs a, uint64_t created, hipStream_t st) {
  const uint32_t W = g->W;
  int rc, bits = 0;
  while (bits < 32 && ((uint64_t)(W - 1) >> bits)) bits++;
  HIP_TRY(hipMemsetAsync(a.wadd, 0, 4ull * W, st));
  launch_gbt_wkey(a, st);
  HIP_TRY(hipGetLastError());
  if ((rc = scan_u32(g, a.wadd, a.wstart, W, &g->ctl()->worker_total, st))) return rc;
  const uint32_t *skeys = nullptr, *svals = nullptr;
  if ((rc = sort_pairs(g, a.keys, a.vals, created, bits, st, &skeys, &svals))) return rc;
  a.keys = const_cast<uint32_t*>(skeys);
  a.vals = const_cast<uint32_t*>(svals);
  launch_gbt_wnum(a, created, st);
  HIP_TRY(hipGetLastError());
  std::vector<uint32_t> add(W);
  GbtWords h{};
  HIP_TRY(hipMemcpyAsync(add.data(), a.wadd, 4ull * W, hipMemcpyDeviceToHost, st));
  if ((rc = read_words(g, h, kGbtWordsError, st))) return rc;
  if (h.error)
    return fail(OSE_EDEVICE, "groupbytrace: device error " + std::to_string(h.error) + " numbering the workers' traces");
  for (uint32_t w = 0; w < W; w++) g->wcnt[w] += add[w];
  return 0;
}

// the rings' OTLP columns, at the first ose_gbt_add_otlp
int otlp_rings(Gbt* g) {
  if (g->omem.p) return 0;
  const GbtOtlpRingLayout L = gbt_otlp_ring_layout(g->pool_cap, g->scope_cap);
  if (int rc = g->omem.need(L.end)) return rc;
  g->O2.msg_len = part_ptr<uint32_t>(g->omem, L.msg_len);
  g->O2.hdr_off = part_ptr<uint64_t>(g->omem, L.hdr_off);
  g->O2.hdr_res = part_ptr<uint32_t>(g->omem, L.hdr_res);
  g->O2.hdr_scope = part_ptr<uint32_t>(g->omem, L.hdr_scope);
  return 0;
}

// ---- ose_gbt_add / ose_gbt_add_otlp, step by step -----------------------------
// the batch's columns, and the room left in the span and scope rings
int add_check(const Gbt* g, const ose_columns* c, const OtlpBatchView* v) {
  const uint64_t n = c->n_spans, S = c->n_scopes;
  if (v) {
    // offsets into the ring and into a release are scanned as uint32
    if (g->arena_cap >= (1ull << 32))
      return fail(OSE_ERANGE, "groupbytrace: an OTLP-fed store takes an arena_capacity below 2^32");
    if (!v->d_spans || !c->arena || (v->res_on_device ? !v->d_res_ref || !v->d_scope_ref
                                                       : v->h_res_n != c->n_resources || v->h_scope_n != S))
      return fail(OSE_EINVAL, "groupbytrace: the OTLP batch has no message layout");
  }
  if (g->K && c->n_attr_keys != g->K) return fail(OSE_EINVAL, "groupbytrace: the batch's attribute key columns differ from the engine's");
  if (c->attr_match && std::max<uint32_t>(1, c->attr_match_words) != g->e->attr_words)
    return fail(OSE_EINVAL, "groupbytrace: attr_match_words differs from the engine's span_attribute rule words");
  if (!c->trace_id || !c->start_ns || !c->end_ns || !c->status || !c->kind || !c->scope || !c->scope_resource ||
      !c->res_svc || !c->res_attrset || (g->K && (!c->attr_type || !c->attr_val)))
    return fail(OSE_EINVAL, "groupbytrace: a required column is NULL");
  if (g->sql && c->db_flags && !c->db_query)   // db_query is read wherever a flag has OSE_DB_HAS_QUERY
    return fail(OSE_EINVAL, "groupbytrace: a required column is NULL (db_flags without db_query)");
  if (g->pool_end - g->pool_begin + n > g->pool_cap || g->scope_end - g->scope_begin + S > g->scope_cap)
    return fail(OSE_ERANGE, "groupbytrace: the store is full (spans waiting for wait_duration exceed its capacity)");
  return 0;
}

// The persistent id table: at least 4x the live traces plus the batch;
// re-inserted from the live traces (*rebuild) when it grows, when tombstones
// and live ids would pass half of it, and when the epoch tag wraps.  Numbers the add.
int add_size_table(Gbt* g, uint64_t n, uint64_t live, hipStream_t st, bool* rebuild_out) {
  uint64_t slots = 1024;
  while (slots < 4 * (live + n)) slots <<= 1;
  bool rebuild = !g->table_valid || g->slots_used + n > g->table_slots / 2;
  if (slots > g->table_slots || g->epoch + 1 >= (1u << 29)) {
    if (int rc = g->table.need(std::max(slots, g->table_slots) * sizeof(GbtSlot))) return rc;
    g->table_slots = std::max(slots, g->table_slots);
    HIP_TRY(hipMemsetAsync(g->table.p, 0, g->table_slots * sizeof(GbtSlot), st));
    g->epoch = 0;
    rebuild = true;
  }
  if (rebuild) g->epoch++;
  g->add_gen = g->add_gen + 1 == 0 ? 1 : g->add_gen + 1;
  *rebuild_out = rebuild;
  return 0;
}

// The add's arguments: the scratch parts, the batch, the ring positions; the
// host-side inputs (attribute-set map, workers' counts, a host-walked batch's
// refs) are queued for the device.  *max_set: the largest stable set id.
int add_args(Gbt* g, const ose_columns* c, const uint32_t* attrset_map, const OtlpBatchView* v, const GbtAddLayout& L,
             uint64_t lo, hipStream_t st, GbtArgs& a, uint32_t* max_set) {
  const uint64_t A = c->n_attrsets, S = c->n_scopes, R = c->n_resources;
  const DevMem& sc = g->scratch;
  a = base_args(g);
  a.slot_of = part_ptr<uint64_t>(sc, L.slot_of);
  a.flag = part_ptr<uint32_t>(sc, L.flag);
  a.rank = part_ptr<uint32_t>(sc, L.rank);
  a.strlen = part_ptr<uint32_t>(sc, L.strlen);
  a.stroff = part_ptr<uint32_t>(sc, L.stroff);
  *max_set = A ? (uint32_t)A - 1 : 0;
  if (attrset_map && A) {
    uint32_t* dmap = part_ptr<uint32_t>(sc, L.attrset_map);
    HIP_TRY(hipMemcpyAsync(dmap, attrset_map, 4 * A, hipMemcpyHostToDevice, st));
    *max_set = *std::max_element(attrset_map, attrset_map + A);
    a.attrset_map = dmap;
  }
  if (g->W > 1) {
    a.keys = part_ptr<uint32_t>(sc, L.keys);
    a.vals = part_ptr<uint32_t>(sc, L.vals);
    if (int rc = upload_worker_counts(g, st)) return rc;
  }
  if (v) {
    a.otlp.hres = part_ptr<uint32_t>(sc, L.hres);
    a.otlp.hscope = part_ptr<uint32_t>(sc, L.hscope);
    a.otlp.hlen = part_ptr<uint32_t>(sc, L.hlen);
    a.otlp.hoff = part_ptr<uint32_t>(sc, L.hoff);
    a.otlp.span_ref = v->d_spans;
    if (v->res_on_device) {
      a.otlp.res_ref = v->d_res_ref;
      a.otlp.scope_ref = v->d_scope_ref;
    } else {   // (pageable sources: the copies are staged before the calls return)
      uint64_t *rr = part_ptr<uint64_t>(sc, L.res_ref), *sr = part_ptr<uint64_t>(sc, L.scope_ref);
      if (R) HIP_TRY(hipMemcpyAsync(rr, v->h_res_ref, 8 * R, hipMemcpyHostToDevice, st));
      if (S) HIP_TRY(hipMemcpyAsync(sr, v->h_scope_ref, 8 * S, hipMemcpyHostToDevice, st));
      a.otlp.res_ref = rr;
      a.otlp.scope_ref = sr;
    }
  }
  a.cols = *c;
  a.n = c->n_spans;
  a.n_scopes = S;
  a.next_seq = g->next_seq;
  a.live_lo = lo;
  a.live_hi = g->next_seq;
  a.add_gen = g->add_gen;
  a.pool_pos = g->pool_end;
  a.scope_pos = g->scope_end;
  a.arena_pos = g->arena_end;
  a.arena_room = g->arena_cap - (g->arena_end - g->arena_begin);
  a.totals = g->ctl()->totals;   // [0] new traces, [1] string bytes
  return 0;
}

// every span's slot in the id table, the new traces' creators, and the scans
// of the creator flags, the string lengths and (OTLP) the header lengths
int add_lookup_and_scans(Gbt* g, const GbtArgs& a, bool rebuild, bool otlp, hipStream_t st) {
  GbtWords* w = g->ctl();
  int rc;
  HIP_TRY(hipMemsetAsync(w, 0, kGbtWordsScans, st));                        // error word, totals
  if (otlp) HIP_TRY(hipMemsetAsync(&w->hdr_total, 0, kGbtWordsOtlp, st));   // header bytes (u32 scan total), all bytes (u64)
  (void)hipGetLastError();
  if (rebuild) launch_gbt_rebuild(a, st);
  launch_gbt_lookup(a, st);
  if (otlp) launch_gbt_hdr_len(a, st);
  launch_gbt_creator(a, st);
  HIP_TRY(hipGetLastError());
  if ((rc = scan_u32(g, a.flag, a.rank, a.n, &w->totals[0], st))) return rc;
  if ((rc = scan_u32(g, a.strlen, a.stroff, a.n, &w->totals[1], st))) return rc;
  if (otlp) {
    if ((rc = scan_u32(g, a.otlp.hlen, a.otlp.hoff, a.n_scopes, &w->hdr_total, st))) return rc;
    launch_gbt_total(a, st);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

// Every kernel here stores nothing when the batch's strings do not fit the
// arena ring (kGbtErrRefused): a refused add leaves the store as it was.
int add_store(Gbt* g, const GbtArgs& a, bool otlp, hipStream_t st) {
  launch_gbt_assign(a, st);
  launch_gbt_append(a, st);
  launch_gbt_scopes(a, st);
  launch_gbt_strings(a, st);
  launch_gbt_query_copy(a, st);   // (a store that carries the SQL columns: the queries, a wave at a time)
  if (otlp) {
    if (g->time_copies) HIP_TRY(hipEventRecord(g->ev[0], st));
    launch_gbt_msg_copy(a, st);   // the Span messages, a wave at a time; the scopes' header blocks
    if (g->time_copies) HIP_TRY(hipEventRecord(g->ev[1], st));
    launch_gbt_hdr_copy(a, st);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// what the control words say of the add, and what that means for the id table
int add_decode(Gbt* g, const GbtWords& h, uint64_t n, uint64_t live, bool rebuild) {
  if (rebuild) g->slots_used = live;
  g->table_valid = true;
  if (h.error & kGbtErrHeader) {   // (nothing stored: the kernels treat it as a refusal)
    g->slots_used += n;
    return fail(OSE_EINVAL, "groupbytrace: a ResourceSpans or ScopeSpans header the store cannot carry (malformed, or a group)");
  }
  if (h.error & kGbtErrRefused) {
    g->slots_used += n;   // ids the lookups claimed stay as tombstones
    return fail(OSE_ERANGE, "groupbytrace: the string arena is full (bytes waiting for wait_duration exceed its capacity)");
  }
  if (h.error) {
    g->table_valid = false;
    return fail(OSE_EDEVICE, "groupbytrace: device table error " + std::to_string(h.error));
  }
  return 0;
}

void add_commit(Gbt* g, const ose_columns* c, int64_t now, uint64_t created, uint64_t bytes, uint32_t max_set) {
  g->slots_used += created;
  g->next_seq += created;
  g->created += created;
  g->added_spans += c->n_spans;
  g->pool_end += c->n_spans;
  g->scope_end += c->n_scopes;
  g->arena_end += bytes;
  g->n_attrsets = std::max<uint32_t>(g->n_attrsets, c->n_attrsets ? max_set + 1 : 0);
  g->epochs.push_back(Gbt::Epoch{now, g->next_seq, g->pool_end, g->scope_end, g->arena_end,
                                 g->W > 1 ? g->wcnt : std::vector<uint64_t>{}});
  g->last_now = now;
}

// v: the decoded batch behind `c` (ose_gbt_add_otlp), NULL for ose_gbt_add
int gbt_add(Gbt* g, const ose_columns* c, const uint32_t* attrset_map, int64_t now, hipStream_t st,
            const OtlpBatchView* v = nullptr) {
  const Gbt::Mode want = v ? Gbt::kOtlp : Gbt::kColumns;
  if (g->mode != Gbt::kUnset && g->mode != want)
    return fail(OSE_EINVAL, v ? "groupbytrace: ose_gbt_add_otlp on a store that ose_gbt_add has fed"
                              : "groupbytrace: ose_gbt_add on a store that ose_gbt_add_otlp has fed");
  if (now < g->last_now) return fail(OSE_EINVAL, "groupbytrace: now_ns went backwards");
  const uint64_t n = c->n_spans, S = c->n_scopes;
  if (!n) return 0;
  int rc;
  if ((rc = add_check(g, c, v))) return rc;
  // An added span joins its id's trace only while that trace is waiting: not
  // released, not evicted, and not past its wait_duration at `now` (contrib's
  // timer would have sent it downstream at its deadline, and later spans of
  // the id start a new trace; the expired one still goes out at the next
  // release).
  const uint64_t lo = std::max(g->live_lo(), g->expired_below(now));
  const uint64_t live = g->next_seq - lo;
  bool rebuild;
  if ((rc = add_size_table(g, n, live, st, &rebuild))) return rc;
  const GbtAddLayout L = gbt_add_layout(n, c->n_attrsets, S, c->n_resources, g->W > 1, v != nullptr);
  if ((rc = g->scratch.need(L.end)) ||
      (rc = words_need(g, std::max<uint64_t>(std::max<uint64_t>(n, g->W), v ? S : 0))) || (v && (rc = otlp_rings(g))))
    return rc;
  const Gbt::Mode mode0 = g->mode;
  g->mode = want;   // base_args picks the instances; put back unless the add succeeds
  struct ModeGuard {
    Gbt* g;
    Gbt::Mode m;
    bool keep = false;
    ~ModeGuard() { if (!keep) g->mode = m; }
  } guard{g, mode0};
  GbtArgs a{};
  uint32_t max_set;
  GbtWords h{};
  if ((rc = add_args(g, c, attrset_map, v, L, lo, st, a, &max_set)) ||
      (rc = add_lookup_and_scans(g, a, rebuild, v != nullptr, st)) || (rc = add_store(g, a, v != nullptr, st)) ||
      (rc = read_words(g, h, v ? kGbtWordsAll : kGbtWordsScans, st)))
    return rc;
  if (v && g->time_copies) HIP_TRY(hipEventElapsedTime(&g->copy_ms[0], g->ev[0], g->ev[1]));
  if ((rc = add_decode(g, h, n, live, rebuild))) return rc;
  const uint64_t created = h.totals[0], bytes = v ? h.total64 : h.totals[1];
  guard.keep = true;
  if (g->W > 1 && created && (rc = number_workers(g, a, created, st))) {
    g->table_valid = false;
    return rc;
  }
  add_commit(g, c, now, created, bytes, max_set);
  return 0;
}

// ---- ose_gbt_release / ose_gbt_release_otlp, step by step ---------------------
// The released batch's columns in slab order: the GbtArgs member the kernels
// write through, the ose_columns member it is published as (kNoCol: one of
// the OTLP layout's, published through OtlpReleasedLayout), its bytes per
// span or fragment (every column has room for a value per released span),
// what they scale with, and the stores that have the column.
enum : uint8_t { kPerItem, kPerAttrWord, kPerKey };      // kPerKey: times K, and 16 bytes more
enum : uint8_t { kAlways, kIfKeys, kIfSql, kIfOtlp };   // kIfKeys: always in the slab, published when K > 0
constexpr size_t kNoCol = ~size_t(0);
struct OutCol { size_t arg, col; uint8_t bytes, scale, when; };
#define COL(member, column, ...) {offsetof(GbtArgs, out.member), offsetof(ose_columns, column), __VA_ARGS__}
#define ANY(member, column, bytes) COL(member, column, bytes, kPerItem, kAlways)
#define OTLP(member, bytes) {offsetof(GbtArgs, otlp.member), kNoCol, bytes, kPerItem, kIfOtlp}
const OutCol kOutCols[] = {
    ANY(tid, trace_id, 16), ANY(start, start_ns, 8), ANY(end, end_ns, 8), COL(attr_match, attr_match, 8, kPerAttrWord, kAlways),
    ANY(status, status, 1), ANY(kind, kind, 1), ANY(url_flags, url_flags, 1), ANY(span_size, span_size, 4),
    ANY(name_len, name_len, 4), ANY(resource, resource, 4), ANY(scope, scope, 4), ANY(route, route, 8), ANY(path, path, 8),
    COL(attr_type, attr_type, 1, kPerKey, kIfKeys), COL(attr_val, attr_val, 8, kPerKey, kIfKeys),
    ANY(res_svc, res_svc, 4), ANY(res_svc_str, res_svc_str, 4), ANY(res_attrset, res_attrset, 4), ANY(res_size, res_size, 4),
    ANY(scope_size, scope_size, 4), ANY(scope_resource, scope_resource, 4), ANY(res_url_ok, res_url_ok, 1),
    COL(db_flags, db_flags, 1, kPerItem, kIfSql), COL(db_query, db_query, 8, kPerItem, kIfSql),
    COL(res_sql_ok, res_sql_ok, 1, kPerItem, kIfSql),
    // what the GPU encoder reads: per span, per fragment (at most m)
    OTLP(out_span_ref, 8), OTLP(out_span0, 4), OTLP(out_res_scope0, 4), OTLP(out_hdr, 8), OTLP(out_schema, 8),
    OTLP(out_res_ref, 8), OTLP(out_scope_ref, 8),
};
#undef COL
#undef ANY
#undef OTLP

// Which epochs have expired at `now` (the first k), the traces [lo, b) the
// release looks at and the `rel` of them it hands out; the others were
// evicted before their timer (dropped, and counted here).
struct Expired {
  size_t k = 0;
  uint64_t b, lo, range, rel;
  std::vector<uint64_t> wrel1;   // W > 1: the workers' counts up to b
};
Expired release_expired(Gbt* g, int64_t now) {
  Expired x;
  x.b = g->rel_end;
  while (x.k < g->epochs.size() && g->epochs[x.k].t + g->wait_ns <= now) x.b = std::max(x.b, g->epochs[x.k++].seq1);
  x.lo = g->live_lo();
  x.range = x.b > x.lo ? x.b - x.lo : 0;
  x.rel = x.range;
  if (g->W == 1) {
    if (x.b > g->rel_end) {
      const uint64_t ev_hi = std::min(x.b, g->evict_below());
      if (ev_hi > g->rel_end) g->evicted += ev_hi - g->rel_end;
    }
  } else if (x.k) {
    // worker w's traces in [rel_end, b) are its numbers [wrel, wrel1); those below w_evicted were evicted
    x.wrel1 = g->epochs[x.k - 1].wcnt1;
    uint64_t ev = 0;
    for (uint32_t w = 0; w < g->W; w++) {
      const uint64_t e = std::min(x.wrel1[w], g->w_evicted(w));
      if (e > g->wrel[w]) ev += e - g->wrel[w];
    }
    g->evicted += ev;
    x.rel = x.range - ev;
  }
  return x;
}

// the window's spans of the released traces, flagged and compacted into (trace, position) pairs; *m of them
int release_compact(Gbt* g, GbtArgs& a, uint64_t window, const Expired& x, hipStream_t st, uint64_t* m) {
  const GbtReleaseLayout L = gbt_release_layout(window);
  int rc;
  if ((rc = g->scratch.need(L.end)) || (rc = words_need(g, window))) return rc;
  a = base_args(g);
  a.flag = part_ptr<uint32_t>(g->scratch, L.flag);
  a.rank = part_ptr<uint32_t>(g->scratch, L.rank);
  a.strlen = part_ptr<uint32_t>(g->scratch, L.strlen);
  a.stroff = part_ptr<uint32_t>(g->scratch, L.stroff);
  a.keys = part_ptr<uint32_t>(g->scratch, L.keys);
  a.vals = part_ptr<uint32_t>(g->scratch, L.vals);
  a.n = window;
  a.pool_pos = g->pool_begin;
  a.rel_lo = x.lo;
  a.rel_hi = x.b;
  HIP_TRY(hipMemsetAsync(g->ctl(), 0, kGbtWordsScans, st));
  if (g->W > 1 && (rc = upload_worker_counts(g, st))) return rc;
  (void)hipGetLastError();
  launch_gbt_flag(a, st);
  HIP_TRY(hipGetLastError());
  if ((rc = scan_u32(g, a.flag, a.rank, window, &g->ctl()->totals[0], st))) return rc;
  launch_gbt_compact(a, st);
  HIP_TRY(hipGetLastError());
  GbtWords h{};
  if ((rc = read_words(g, h, kGbtWordsCount, st))) return rc;
  if (h.error) return fail(OSE_EDEVICE, "groupbytrace: device error " + std::to_string(h.error));
  *m = h.totals[0];
  return 0;
}

// the released batch of m spans: fixed columns and fragment heads (kOutCols), then strings and fragments
int release_place(Gbt* g, GbtArgs& a, uint64_t m, bool otlp) {
  const uint64_t M = std::max<uint64_t>(m, 1);
  std::vector<SlabPart> parts;
  for (const OutCol& col : kOutCols) {
    if ((col.when == kIfSql && !g->sql) || (col.when == kIfOtlp && !otlp)) continue;
    const size_t bytes = col.scale == kPerKey ? col.bytes * g->K * M + 16
                                              : col.bytes * M * (col.scale == kPerAttrWord ? g->e->attr_words : 1);
    parts.push_back({reinterpret_cast<void**>(reinterpret_cast<uint8_t*>(&a) + col.arg), bytes});
  }
  const size_t arena_at = slab_size(parts).total;
  // the strings of the released spans are at most the live arena bytes
  // (OTLP: a header block leaves once per released fragment, so the live
  // bytes are no bound; the message buffer is the released batch's own and
  // is sized from the fragment scan: release_gather)
  const size_t arena_bound = otlp ? 0 : g->arena_end - g->arena_begin;
  // OSE_STAGE_SQLOP reads db_query through 16-byte windows (sqlop_kernel's
  // ByteReader): it needs a 16-byte aligned arena base and 16 readable
  // bytes after arena_bytes.  arena_at is a multiple of 256 in a 256-byte
  // aligned allocation, and 64 bytes follow the last string.
  if (int rc = g->out.need(arena_at + up(arena_bound + 64))) return rc;
  slab_assign(parts, g->out.p);
  a.out.arena = g->out.p + arena_at;
  return 0;
}

// The released spans' columns in `order`, the scans of their fragment flags
// and string lengths; OTLP: the message buffer sized from the 64-bit byte
// total (*msg_bytes) and the fragments (*frags), read before a byte moves.
int release_gather(Gbt* g, GbtArgs& a, uint64_t m, bool otlp, hipStream_t st, uint64_t* msg_bytes, uint32_t* frags) {
  GbtWords* w = g->ctl();
  int rc;
  HIP_TRY(hipMemsetAsync(w, 0, kGbtWordsScans, st));
  launch_gbt_gather(a, st);
  HIP_TRY(hipGetLastError());
  if ((rc = scan_u32(g, a.flag, a.rank, m, &w->totals[0], st))) return rc;       // fragments
  if ((rc = scan_u32(g, a.strlen, a.stroff, m, &w->totals[1], st))) return rc;   // string offsets
  if (!otlp) return 0;
  HIP_TRY(hipMemsetAsync(a.otlp.total64, 0, 8, st));
  a.n_scopes = 0;
  launch_gbt_total(a, st);
  HIP_TRY(hipGetLastError());
  GbtWords h{};
  if ((rc = read_words(g, h, kGbtWordsAll, st))) return rc;
  if (h.error) return fail(OSE_EDEVICE, "groupbytrace: device error " + std::to_string(h.error));
  *frags = h.totals[0];
  *msg_bytes = h.total64;
  if (*msg_bytes > 0xFFFFFF00ull)   // the u32 offsets above have wrapped: nothing is moved
    return fail(OSE_ERANGE, "groupbytrace: the released messages exceed the 4 GiB a batch's refs can address");
  if ((rc = otlp_released_arena(g->rel, up(*msg_bytes + 64), &a.out.arena))) return rc;
  HIP_TRY(hipMemsetAsync(a.out.arena + *msg_bytes, 0, 64, st));
  return 0;
}

// the fragment columns and the string blocks; h: the error word and both totals afterwards
int release_emit(Gbt* g, const GbtArgs& a, bool otlp, uint32_t frags, hipStream_t st, GbtWords& h) {
  launch_gbt_emit(a, st);
  if (otlp && g->time_copies) HIP_TRY(hipEventRecord(g->ev[2], st));
  launch_gbt_block_copy(a, st);   // (a store that carries the SQL columns: emit leaves the bytes to it)
  if (otlp && g->time_copies) HIP_TRY(hipEventRecord(g->ev[3], st));
  if (otlp) launch_gbt_frag_hdr(a, frags, st);
  HIP_TRY(hipGetLastError());
  if (int rc = read_words(g, h, kGbtWordsTotals, st)) return rc;
  if (otlp && g->time_copies) HIP_TRY(hipEventElapsedTime(&g->copy_ms[1], g->ev[2], g->ev[3]));
  if (h.error) return fail(OSE_EDEVICE, "groupbytrace: device error " + std::to_string(h.error));
  return 0;
}

// out_cols: m spans in F fragments (each its own resource and scope), `bytes` of strings or messages
void release_publish(Gbt* g, const GbtArgs& a, uint64_t m, uint32_t F, uint32_t bytes) {
  ose_columns& oc = g->out_cols;
  oc.n_spans = m;
  oc.n_resources = F;
  oc.n_scopes = F;
  oc.n_attrsets = g->n_attrsets;
  oc.attr_match_words = g->e->attr_words;
  oc.n_attr_keys = g->K;
  oc.arena = a.out.arena;
  oc.arena_bytes = bytes;
  for (const OutCol& col : kOutCols)
    if (col.col != kNoCol && !(col.when == kIfSql && !g->sql) && !(col.when == kIfKeys && !g->K))
      std::memcpy(reinterpret_cast<uint8_t*>(&oc) + col.col, reinterpret_cast<const uint8_t*>(&a) + col.arg, sizeof(void*));
}

// the counters, and the rings past every span of an expired epoch (it belongs to a released or evicted trace)
void release_advance(Gbt* g, Expired& x, uint64_t m) {
  g->released += x.rel;
  g->released_spans += m;
  g->rel_end = std::max(g->rel_end, x.b);
  if (!x.k) return;
  if (g->W > 1) g->wrel = std::move(x.wrel1);
  const Gbt::Epoch& last = g->epochs[x.k - 1];
  g->pool_begin = last.pool1;
  g->scope_begin = last.scope1;
  g->arena_begin = last.arena1;
  g->epochs.erase(g->epochs.begin(), g->epochs.begin() + (long)x.k);
}

// otlp: ose_gbt_release_otlp (the released batch g->rel gets the columns and the layout)
int gbt_release(Gbt* g, int64_t now, hipStream_t st, uint32_t* n_traces, bool otlp = false) {
  if (now < g->last_now) return fail(OSE_EINVAL, "groupbytrace: now_ns went backwards");
  g->last_now = now;
  g->out_cols = ose_columns{};
  *n_traces = 0;
  if (otlp) otlp_released_set(g->rel, g->out_cols, OtlpReleasedLayout{});   // an empty batch unless spans leave below
  Expired x = release_expired(g, now);
  const uint64_t window = g->pool_end - g->pool_begin;
  int rc;
  uint64_t m = 0;
  if (x.rel && window) {
    GbtArgs a{};
    if ((rc = release_compact(g, a, window, x, st, &m))) return rc;
    // stable sort of the released spans by trace (window order = arrival order)
    int bits = 0;
    while (bits < 32 && ((x.range - 1) >> bits)) bits++;
    const uint32_t *order = a.vals, *skeys = a.keys;
    if ((rc = sort_pairs(g, a.keys, a.vals, m, bits, st, &skeys, &order)) || (rc = release_place(g, a, m, otlp))) return rc;
    a.n = m;
    a.order = order;
    uint64_t msg_bytes = 0;
    uint32_t frags = 0;
    GbtWords h{};
    if ((rc = release_gather(g, a, m, otlp, st, &msg_bytes, &frags)) || (rc = release_emit(g, a, otlp, frags, st, h)))
      return rc;
    release_publish(g, a, m, h.totals[0], otlp ? (uint32_t)msg_bytes : h.totals[1]);
    if (otlp) {
      const GbtOtlp& X = a.otlp;
      otlp_released_set(g->rel, g->out_cols,
                        OtlpReleasedLayout{X.out_span_ref, X.out_span0, X.out_hdr, X.out_schema, X.out_res_ref,
                                           X.out_res_scope0, X.out_scope_ref});
    }
  }
  *n_traces = (uint32_t)x.rel;   // traces with spans in the window (every released trace has >= 1)
  release_advance(g, x, m);
  return 0;
}
}  // namespace

}  // namespace ose

using namespace ose;

extern "C" {

int ose_gbt_create(ose_engine* eng, const char* cfg_json, uint64_t span_capacity, uint64_t arena_capacity,
                   ose_gbt** out) {
  if (!eng || !cfg_json || !out) return fail(OSE_EINVAL, "NULL argument");
  Engine* e = reinterpret_cast<Engine*>(eng);
  if (int rc = bind_device(e)) return rc;
  auto* g = new Gbt();
  g->e = e;
  try {
    const Json cfg = parse_json(cfg_json);
    std::string wait = "1s";   // the processor's default (contrib); Odigos sets "30s"
    if (const Json* w = cfg.get("wait_duration")) {
      if (!w->is_str()) { delete g; return fail(OSE_EINVAL, "wait_duration: expected a duration string"); }
      wait = w->s;
    }
    if (!parse_go_duration(wait, g->wait_ns)) { delete g; return fail(OSE_EINVAL, "time: invalid duration \"" + wait + "\""); }
    if (const Json* nt = cfg.get("num_traces")) g->num_traces = (uint64_t)nt->i64();
    int64_t nw = 1;
    if (const Json* w = cfg.get("num_workers")) nw = w->i64();
    if ((int64_t)g->num_traces <= 0) { delete g; return fail(OSE_EINVAL, "groupbytrace: num_traces must be positive"); }
    if (nw <= 0 || nw > (1 << 20)) { delete g; return fail(OSE_EINVAL, "groupbytrace: num_workers must be in [1, 2^20]"); }
    // each worker's ring holds num_traces / num_workers ids (contrib's
    // newRingBuffer would divide by zero below one)
    if ((uint64_t)nw > g->num_traces) { delete g; return fail(OSE_EINVAL, "groupbytrace: num_traces must be at least num_workers"); }
    g->W = (uint32_t)nw;
  } catch (const std::exception& ex) {
    delete g;
    return fail(OSE_EINVAL, ex.what());
  }
  g->K = (uint32_t)e->attr_keys.size();
  g->sql = e->has_sqlop;
  g->pool_cap = std::max<uint64_t>(span_capacity, 1024);
  g->scope_cap = g->pool_cap;
  g->arena_cap = std::max<uint64_t>(arena_capacity, 1 << 16);
  // one worker: the ring is num_traces ids (every live seq is within
  // num_traces of the newest).  W > 1: a worker's old trace can outlive
  // num_traces newer ones of other workers, but every seq not yet released
  // has its first span in the pool, so pool_cap slots cover them
  g->wcap = g->num_traces / g->W;
  g->ring_n = g->W == 1 ? g->num_traces : g->pool_cap;
  g->wcnt.assign(g->W, 0);
  g->wrel.assign(g->W, 0);
  const uint64_t C = g->pool_cap, K = g->K;
  std::vector<SlabPart> parts = {
      {(void**)&g->P.tid, 16 * C}, {(void**)&g->P.start, 8 * C}, {(void**)&g->P.end, 8 * C},
      {(void**)&g->P.attr_match, 8 * C * g->e->attr_words}, {(void**)&g->P.seq, 8 * C}, {(void**)&g->P.origin, 8 * C},
      {(void**)&g->P.str_off, 8 * C}, {(void**)&g->P.status, C}, {(void**)&g->P.kind, C},
      {(void**)&g->P.url_flags, C}, {(void**)&g->P.span_size, 4 * C}, {(void**)&g->P.name_len, 4 * C},
      {(void**)&g->P.route, 8 * C}, {(void**)&g->P.path, 8 * C}, {(void**)&g->P.attr_type, K * C + 16},
      {(void**)&g->P.attr_val, 8 * K * C + 16},
  };
  if (g->sql) parts.insert(parts.end(), {{(void**)&g->P.db_flags, C}, {(void**)&g->P.db_query, 8 * C}});
  const uint64_t SC = g->scope_cap;
  std::vector<SlabPart> sparts = {
      {(void**)&g->Q.res_svc, 4 * SC}, {(void**)&g->Q.res_svc_str, 4 * SC}, {(void**)&g->Q.res_attrset, 4 * SC},
      {(void**)&g->Q.res_size, 4 * SC}, {(void**)&g->Q.scope_size, 4 * SC}, {(void**)&g->Q.res_url_ok, SC},
  };
  if (g->sql) sparts.push_back({(void**)&g->Q.res_sql_ok, SC});
  int rc;
  if ((rc = g->pool.need(slab_size(parts).total)) || (rc = g->scopes.need(slab_size(sparts).total)) ||
      (rc = g->arena.need(g->arena_cap)) || (rc = g->ring.need(16 * g->ring_n)) || (rc = g->words.need(1 << 16)) ||
      (g->W > 1 && ((rc = g->tinfo.need(8 * g->ring_n)) || (rc = g->wdev.need(gbt_worker_layout(g->W).end))))) {
    delete g;
    return rc;
  }
  slab_assign(parts, g->pool.p);
  slab_assign(sparts, g->scopes.p);
  engine_retain(e);   // dropped by ose_gbt_destroy
  *out = reinterpret_cast<ose_gbt*>(g);
  return 0;
}

void ose_gbt_destroy(ose_gbt* gg) {
  if (!gg) return;
  LastErrorScope keep("ose_gbt_destroy");
  auto* g = reinterpret_cast<Gbt*>(gg);
  Engine* e = g->e;
  (void)bind_device(e);
  delete g;
  engine_unref(e);
}

int ose_gbt_add(ose_gbt* gg, const ose_columns* cols, const uint32_t* attrset_map, int64_t now_ns, void* hip_stream) {
  if (!gg || !cols) return fail(OSE_EINVAL, "NULL argument");
  auto* g = reinterpret_cast<Gbt*>(gg);
  if (int rc = bind_device(g->e)) return rc;
  return gbt_add(g, cols, attrset_map, now_ns, static_cast<hipStream_t>(hip_stream));
}

int ose_gbt_add_otlp(ose_gbt* gg, const ose_otlp_batch* b, const uint32_t* attrset_map, int64_t now_ns,
                     void* hip_stream) {
  if (!gg || !b) return fail(OSE_EINVAL, "NULL argument");
  auto* g = reinterpret_cast<Gbt*>(gg);
  OtlpBatchView v;
  otlp_batch_view(b, &v);
  if (v.e != g->e) return fail(OSE_EINVAL, "groupbytrace: the batch belongs to another engine");
  if (v.released) return fail(OSE_EINVAL, "groupbytrace: a released batch cannot be added");
  if (int rc = bind_device(g->e)) return rc;
  return gbt_add(g, v.cols, attrset_map, now_ns, static_cast<hipStream_t>(hip_stream), &v);
}

int ose_gbt_release_otlp(ose_gbt* gg, int64_t now_ns, void* hip_stream, const ose_otlp_batch** out,
                         uint32_t* n_traces) {
  if (!gg || !out || !n_traces) return fail(OSE_EINVAL, "NULL argument");
  auto* g = reinterpret_cast<Gbt*>(gg);
  if (g->mode == Gbt::kColumns)
    return fail(OSE_EINVAL, "groupbytrace: ose_gbt_release_otlp on a store that ose_gbt_add has fed (use ose_gbt_release)");
  if (int rc = bind_device(g->e)) return rc;
  if (!g->rel) g->rel = otlp_released_new(g->e);
  const int rc = gbt_release(g, now_ns, static_cast<hipStream_t>(hip_stream), n_traces, true);
  *out = g->rel;
  return rc;
}

int ose_gbt_release(ose_gbt* gg, int64_t now_ns, void* hip_stream, const ose_columns** out, uint32_t* n_traces) {
  if (!gg || !out || !n_traces) return fail(OSE_EINVAL, "NULL argument");
  auto* g = reinterpret_cast<Gbt*>(gg);
  if (g->mode == Gbt::kOtlp)
    return fail(OSE_EINVAL, "groupbytrace: ose_gbt_release on a store that ose_gbt_add_otlp has fed (use ose_gbt_release_otlp)");
  if (int rc = bind_device(g->e)) return rc;
  const int rc = gbt_release(g, now_ns, static_cast<hipStream_t>(hip_stream), n_traces);
  *out = &g->out_cols;
  return rc;
}

int ose_gbt_stats(const ose_gbt* gg, uint64_t* out8) {
  if (!gg || !out8) return fail(OSE_EINVAL, "NULL argument");
  const auto* g = reinterpret_cast<const Gbt*>(gg);
  out8[0] = g->waiting();                         // traces waiting
  out8[1] = g->pool_end - g->pool_begin;          // spans held (waiting or released, not yet reclaimed)
  out8[2] = g->created;
  out8[3] = g->released;
  out8[4] = g->evicted;
  out8[5] = g->released_spans;
  out8[6] = g->added_spans;
  out8[7] = g->arena_end - g->arena_begin;
  return 0;
}

// copies every column of the last release whose dst pointer is non-NULL
int ose_gbt_download(const ose_gbt* gg, const ose_columns* dst) {
  if (!gg || !dst) return fail(OSE_EINVAL, "NULL argument");
  const auto* g = reinterpret_cast<const Gbt*>(gg);
  if (g->mode == Gbt::kOtlp)
    return fail(OSE_EINVAL, "groupbytrace: ose_gbt_download on a store that ose_gbt_add_otlp has fed (use ose_otlp_download)");
  if (int rc = bind_device(g->e)) return rc;
  return download_columns(g->out_cols, dst);
}

// Diagnostics (tools/gbt_otlp_bench.py): on != 0 turns on HIP events around an
// OTLP-fed store's two wave copies; ms2 (may be NULL) receives the time of
// gbt_msg_copy_kernel in the last add and of gbt_block_copy_kernel in the
// last release
int osehost_gbt_copy_times(ose_gbt* gg, int on, double* ms2) {
  if (!gg) return fail(OSE_EINVAL, "NULL argument");
  auto* g = reinterpret_cast<Gbt*>(gg);
  if (int rc = bind_device(g->e)) return rc;
  if (on)
    for (hipEvent_t& e : g->ev)
      if (!e) HIP_TRY(hipEventCreate(&e));
  g->time_copies = on != 0;
  if (ms2) {
    ms2[0] = g->copy_ms[0];
    ms2[1] = g->copy_ms[1];
  }
  return 0;
}

// Test seam (tests/gbt_layouts.py): the host's bookkeeping, so that a layout
// proves the growth, the rebuild or the wrap it was laid for.  Reads host
// fields only: nothing is launched, nothing changes.  out[0, min(n, 13)):
// table_slots, epoch, slots_used, pool_begin, pool_end, scope_begin,
// scope_end, arena_begin, arena_end, next_seq, rel_end, epochs, n_attrsets.
// Returns the number of fields there are.
int osehost_gbt_state(const ose_gbt* gg, uint64_t* out, uint32_t n) {
  if (!gg || !out) return fail(OSE_EINVAL, "NULL argument");
  const auto* g = reinterpret_cast<const Gbt*>(gg);
  const uint64_t v[] = {g->table_slots, g->epoch,       g->slots_used, g->pool_begin, g->pool_end,
                        g->scope_begin, g->scope_end,   g->arena_begin, g->arena_end, g->next_seq,
                        g->rel_end,     g->epochs.size(), g->n_attrsets};
  const uint32_t have = (uint32_t)(sizeof(v) / sizeof(v[0]));
  for (uint32_t k = 0; k < std::min(n, have); k++) out[k] = v[k];
  return (int)have;
}

// Test seam (tests/test_gbt_host_layout.py), no device: one of the store's
// layouts (gbt_layout.hpp), part by part in its struct's order; returns the
// number of parts, 0 for an unknown `which`.  0: the add scratch (n spans); 1:
// the release scratch (n: the window); 2: the sort buffer (n pairs); 3: the
// OTLP ring columns (n: the pool capacity, n_scopes: the scope ring's); 4: wdev.
uint32_t osehost_gbt_layout(uint32_t which, uint64_t n, uint64_t n_attrsets, uint64_t n_scopes, uint64_t n_resources,
                            uint32_t workers, int otlp, uint64_t* off, uint64_t* bytes, uint32_t cap, uint64_t* end) {
  switch (which) {
    case 0:
      return layout_parts(gbt_add_layout(n, n_attrsets, n_scopes, n_resources, workers > 1, otlp != 0), off, bytes, cap, end);
    case 1: return layout_parts(gbt_release_layout(n), off, bytes, cap, end);
    case 2: return layout_parts(gbt_sort_layout(n, (n + kSortTile - 1) / kSortTile), off, bytes, cap, end);
    case 3: return layout_parts(gbt_otlp_ring_layout(n, n_scopes), off, bytes, cap, end);
    case 4: return layout_parts(gbt_worker_layout(workers), off, bytes, cap, end);
  }
  return 0;
}

// Test seam (CPU): Go's time.ParseDuration as the store reads wait_duration
int osehost_parse_duration(const char* s, int64_t* out) {
  if (!s || !out) return fail(OSE_EINVAL, "NULL argument");
  return parse_go_duration(s, *out) ? 0 : fail(OSE_EINVAL, std::string("time: invalid duration \"") + s + "\"");
}

}  // extern "C"
