// engine.cpp — the C ABI (include/odigos_amd.h): config decoding/validation,
// the workspace, stream and event pools, and run_stages, which places the
// stages of one call in its workspace and queues them in gateway order (each
// stage's tables and launches are in its own *_host.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/odigos_amd.h"
#include "config.hpp"
#include "devcfg.hpp"
#include "engine_internal.hpp"
#include "kernels.hpp"
#include "slab.hpp"

namespace ose {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

// ---------------- engine ----------------
Engine::~Engine() {
  release_exchange_scratch(this);
  release_batch_pool(this);
  release_otlp(this);
  release_encode(this);
  release_condattr(this);
  for (auto& t : timings) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
  for (auto s : streams) (void)hipStreamDestroy(s);
  for (auto ev : event_pool) (void)hipEventDestroy(ev);
  if (url_blob_dev) (void)hipFree(url_blob_dev);
  if (url_blob_forced_dev) (void)hipFree(url_blob_forced_dev);
  for (auto* d : sampling_chunks_dev)
    if (d) (void)hipFree(d);   // (sampling_blob_dev is the first)
  for (auto* d : sampling_svc_map_dev)
    if (d) (void)hipFree(d);
  if (sampling_svc_maps_dev) (void)hipFree(sampling_svc_maps_dev);
  if (shard_tables_dev) (void)hipFree(shard_tables_dev);
  if (path_count_dev) (void)hipFree(path_count_dev);
  if (attr_blob_dev) (void)hipFree(attr_blob_dev);
  if (attr_host_mask_dev) (void)hipFree(attr_host_mask_dev);
  for (auto* w : pool) delete w;
}

Workspace::~Workspace() {
  if (dev) (void)hipFree(dev);
  if (table) (void)hipFree(table);
  if (dup_bkt) (void)hipFree(dup_bkt);
  if (dup_bkt_count) (void)hipFree(dup_bkt_count);
  if (runs) (void)hipFree(runs);
  if (run_count) (void)hipFree(run_count);
  if (attr_bits) (void)hipFree(attr_bits);
  if (ep_planes) (void)hipFree(ep_planes);
  if (svc_local) (void)hipFree(svc_local);
  for (void* f : fold)
    if (f) (void)hipFree(f);
  if (dup_host) (void)hipHostFree(dup_host);
  for (hipEvent_t ev : {pending, dup_ready, fork, join, join2, fork2})
    if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : slice_ev)
    if (ev) (void)hipEventDestroy(ev);
}

hipEvent_t Engine::take_event() {
  if (!event_pool.empty()) {
    hipEvent_t ev = event_pool.back();
    event_pool.pop_back();
    return ev;
  }
  hipEvent_t ev = nullptr;
  (void)hipEventCreate(&ev);
  return ev;
}
Engine::Timed Engine::prof_begin(const char* name, hipStream_t st) {
  std::lock_guard<std::mutex> g(mu);
  Timed t{name, take_event(), take_event()};
  (void)hipEventRecord(t.a, st);
  return t;
}
void Engine::prof_end(Timed& t, hipStream_t st) {
  (void)hipEventRecord(t.b, st);
  std::lock_guard<std::mutex> g(mu);
  timings.push_back(t);
}
void Engine::prof_drop(Timed& t) {
  std::lock_guard<std::mutex> g(mu);
  event_pool.push_back(t.a);
  event_pool.push_back(t.b);
}
int Engine::launch_status() {
  HIP_TRY(hipGetLastError());
  return 0;
}

// True while `st` is being captured into a hipGraph.
bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// Stream-ordered pool: work enqueued on a workspace may still be running
// when the call returns (ose_process_device is asynchronous), so release
// records an event on the caller's stream and the next user of that
// workspace makes its own stream wait for it.  A call captured into a
// hipGraph takes a workspace out of the pool for good: the graph replays
// into it whenever it is launched, so no later call may share it (and no
// event recorded outside the capture may be waited on inside it).
Workspace* Engine::acquire_ws(hipStream_t st) {
  if (stream_capturing(st)) {
    std::lock_guard<std::mutex> g(mu);
    Workspace* w = nullptr;
    if (!free_ws.empty()) {   // the largest free one (ose_reserve sized it)
      auto it = std::max_element(free_ws.begin(), free_ws.end(),
                                 [](const Workspace* a, const Workspace* b) { return a->cap < b->cap; });
      w = *it;
      free_ws.erase(it);
    } else {
      w = new Workspace();
      pool.push_back(w);
    }
    w->captured = true;
    return w;
  }
  Workspace* w = nullptr;
  {
    std::lock_guard<std::mutex> g(mu);
    if (!free_ws.empty()) {
      w = free_ws.back();
      free_ws.pop_back();
    } else {
      w = new Workspace();
      pool.push_back(w);
    }
  }
  if (w->pending_set) (void)hipStreamWaitEvent(st, w->pending, 0);
  return w;
}
// A workspace taken for a capture that queued nothing goes back to the pool.
void Engine::return_unused_ws(Workspace* w) {
  std::lock_guard<std::mutex> g(mu);
  w->captured = false;
  free_ws.push_back(w);
}
void Engine::release_ws(Workspace* w, hipStream_t st) {
  if (w->captured) return;   // owned by the graph it was captured into
  if (!w->pending) (void)hipEventCreateWithFlags(&w->pending, hipEventDisableTiming);
  w->pending_set = w->pending && hipEventRecord(w->pending, st) == hipSuccess;
  std::lock_guard<std::mutex> g(mu);
  free_ws.push_back(w);
}
#ifndef OSE_SIDE_STREAM_PRIO
#define OSE_SIDE_STREAM_PRIO 0
#endif
hipStream_t Engine::take_stream() {
  std::lock_guard<std::mutex> g(mu);
  if (!free_streams.empty()) {
    hipStream_t s = free_streams.back();
    free_streams.pop_back();
    return s;
  }
  hipStream_t s = nullptr;
#if OSE_SIDE_STREAM_PRIO   // A/B: the pool's streams at the greatest priority (profiles/tail_parts_ab.txt)
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest) != hipSuccess) return nullptr;
#else
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
#endif
  streams.push_back(s);
  return s;
}
void Engine::give_stream(hipStream_t s) {
  std::lock_guard<std::mutex> g(mu);
  free_streams.push_back(s);
}

int Workspace::reserve(size_t bytes) {
  if (bytes <= cap) return 0;
  if (captured) return fail(OSE_ENOMEM, "workspace too small inside a hipGraph capture: call ose_reserve first");
  if (dev) HIP_TRY(hipFree(dev));
  dev = nullptr;
  cap = 0;
  size_t want = std::max<size_t>(bytes, 1 << 20);
  HIP_TRY(hipMalloc(&dev, want));
  cap = want;
  return 0;
}

int ensure_device() {
  static int status = 1;   // 1 = unknown
  static std::mutex m;
  std::lock_guard<std::mutex> g(m);
  if (status == 1) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    status = (e == hipSuccess && n > 0) ? 0 : OSE_EDEVICE;
  }
  if (status) return fail(OSE_EDEVICE, "no HIP device visible: the odigos_amd engine runs only on an MI355X (gfx950)");
  return 0;
}

int bind_device(const Engine* e) {
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != e->device) HIP_TRY(hipSetDevice(e->device));
  return 0;
}

static std::mutex g_dropped_mu;
static uint64_t g_dropped_count = 0;
static std::string g_dropped_last;
void note_dropped_error(const char* where, hipError_t err) {
  std::lock_guard<std::mutex> g(g_dropped_mu);
  g_dropped_count++;
  g_dropped_last = std::string(where) + ": " + hipGetErrorName(err) + " (" + hipGetErrorString(err) + ")";
}

void engine_retain(Engine* e) { e->refs.fetch_add(1, std::memory_order_relaxed); }

void engine_unref(Engine* e) {
  if (e->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  LastErrorScope keep("engine_unref");
  (void)bind_device(e);
  (void)hipDeviceSynchronize();   // nothing in flight may still use the buffers freed below
  delete e;
}

int upload(const std::vector<uint8_t>& host, uint8_t** dev) {
  HIP_TRY(hipMalloc(dev, host.size()));
  HIP_TRY(hipMemcpy(*dev, host.data(), host.size(), hipMemcpyHostToDevice));
  return 0;
}

int download_columns(const ose_columns& c, const ose_columns* dst) {
  const uint64_t n = c.n_spans, R = c.n_resources, S = c.n_scopes, K = c.n_attr_keys;
  struct F { const void* src; void* dst; size_t bytes; };
  const F fs[] = {
      {c.arena, (void*)dst->arena, c.arena_bytes}, {c.trace_id, (void*)dst->trace_id, 16 * n},
      {c.start_ns, (void*)dst->start_ns, 8 * n}, {c.end_ns, (void*)dst->end_ns, 8 * n},
      {c.status, (void*)dst->status, n}, {c.kind, (void*)dst->kind, n}, {c.resource, (void*)dst->resource, 4 * n},
      {c.scope, (void*)dst->scope, 4 * n}, {c.url_flags, (void*)dst->url_flags, n}, {c.path, (void*)dst->path, 8 * n},
      {c.route, (void*)dst->route, 8 * n}, {c.span_size, (void*)dst->span_size, 4 * n},
      {c.name_len, (void*)dst->name_len, 4 * n},
      {c.attr_match, (void*)dst->attr_match, 8 * n * std::max<uint32_t>(1, c.attr_match_words)},
      {c.res_svc, (void*)dst->res_svc, 4 * R}, {c.res_svc_str, (void*)dst->res_svc_str, 4 * R},
      {c.res_url_ok, (void*)dst->res_url_ok, R}, {c.res_attrset, (void*)dst->res_attrset, 4 * R},
      {c.res_size, (void*)dst->res_size, 4 * R}, {c.scope_size, (void*)dst->scope_size, 4 * S},
      {c.scope_resource, (void*)dst->scope_resource, 4 * S}, {c.attr_type, (void*)dst->attr_type, K * n},
      {c.attr_val, (void*)dst->attr_val, 8 * K * n}, {c.db_flags, (void*)dst->db_flags, n},
      {c.db_query, (void*)dst->db_query, 8 * n}, {c.res_sql_ok, (void*)dst->res_sql_ok, R},
  };
  for (auto& f : fs)
    if (f.src && f.dst && f.bytes) HIP_TRY(hipMemcpy(f.dst, f.src, f.bytes, hipMemcpyDefault));
  return 0;
}

namespace {
// what run_stages refuses before anything is queued
int check_stage_mask(const Engine* e, const ose_columns* c, const ose_outputs* o, uint32_t mask) {
  if (mask & OSE_STAGE_CONDATTR) return refuse_condattr("ose_process and ose_process_device");
  if (mask & ~(OSE_STAGE_SAMPLE | OSE_STAGE_TEMPLATE | OSE_STAGE_SIZE | OSE_STAGE_APPLY_KEEP | OSE_STAGE_TEMPLATE_REFS |
               OSE_STAGE_APPLY_TEMPLATE | OSE_STAGE_SQLOP | OSE_STAGE_APPLY_SQLOP))
    return fail(OSE_EINVAL, "unknown stage bit");
  if ((mask & OSE_STAGE_TEMPLATE_REFS) && !(mask & OSE_STAGE_TEMPLATE))
    return fail(OSE_EINVAL, "OSE_STAGE_TEMPLATE_REFS needs OSE_STAGE_TEMPLATE");
  if ((mask & OSE_STAGE_APPLY_KEEP) && (mask & OSE_STAGE_SAMPLE))
    return fail(OSE_EINVAL, "OSE_STAGE_APPLY_KEEP and OSE_STAGE_SAMPLE exclude each other");
  if ((mask & OSE_STAGE_APPLY_TEMPLATE) && (mask & OSE_STAGE_TEMPLATE))
    return fail(OSE_EINVAL, "OSE_STAGE_APPLY_TEMPLATE and OSE_STAGE_TEMPLATE exclude each other");
  if ((mask & OSE_STAGE_APPLY_SQLOP) && (mask & OSE_STAGE_SQLOP))
    return fail(OSE_EINVAL, "OSE_STAGE_APPLY_SQLOP and OSE_STAGE_SQLOP exclude each other");
  // odigossqldboperationprocessor: refused before anything is queued
  if (mask & OSE_STAGE_SQLOP) {
    if (!e->has_sqlop) return fail(OSE_EINVAL, "odigossqldboperationprocessor is not configured on this engine");
    if (!c->db_flags || !c->db_query || !c->resource || !o->sql_op)
      return fail(OSE_EINVAL, "SQLOP stage needs db_flags, db_query, resource and sql_op");
  }
  return 0;
}

// The side stream the URL front runs on beside the trace stage, and its joins
// with the caller's stream.
struct UrlFork {
  Engine* e;
  Workspace* ws;
  hipStream_t st;                // the caller's stream
  hipStream_t ust = nullptr;     // the side stream (nullptr: no fork, the URL front runs on st)
  bool early_join = false;       // ws->join is recorded inside run_url, behind the two plan kernels
  bool join_recorded = false;    // ... and was: the side stream is joined a second time at the end
  void open() {
    if (!ws->fork) (void)hipEventCreateWithFlags(&ws->fork, hipEventDisableTiming);
    if (!ws->join) (void)hipEventCreateWithFlags(&ws->join, hipEventDisableTiming);
    if (!ws->join2) (void)hipEventCreateWithFlags(&ws->join2, hipEventDisableTiming);
    // (the fork stream's priority, high or low, measured no different:
    // profiles/r6u_url_stream_priority_ab.txt)
    if (ws->fork && ws->join && ws->join2) ust = e->take_stream();
    if (ust && (hipEventRecord(ws->fork, st) != hipSuccess || hipStreamWaitEvent(ust, ws->fork, 0) != hipSuccess)) {
      e->give_stream(ust);
      ust = nullptr;
    }
  }
  // the caller's stream waits for the side stream at `ev` (recorded: it was
  // recorded there already); rc takes the failure if it holds none yet
  void join(hipEvent_t ev, bool recorded, int& rc) {
    const hipError_t je = recorded ? hipSuccess : hipEventRecord(ev, ust);
    const hipError_t jw = je == hipSuccess ? hipStreamWaitEvent(st, ev, 0) : je;
    if (jw != hipSuccess) {   // cannot order the streams: wait for the URL work on the host
      (void)hipStreamSynchronize(ust);
      if (ust2) (void)hipStreamSynchronize(ust2);
      if (!rc) rc = fail(OSE_EDEVICE, std::string("URL stream join: ") + hipGetErrorString(jw));
    }
  }
  // The plan in K slices (kernels.hpp UrlSlices): an event per slice, and for
  // the staggered form a second side stream and the event it starts behind.
  // Returns the slices the call can have (1 when an event is missing; a
  // staggered call without its second stream runs its slices in order).
  hipStream_t ust2 = nullptr;
  uint32_t open_slices(uint32_t k, uint32_t form) {
    static_assert(sizeof(ws->slice_ev) / sizeof(ws->slice_ev[0]) == kUrlMaxSlices, "an event per slice");
    if (k > kUrlMaxSlices) k = kUrlMaxSlices;
    for (uint32_t s = 0; s < k; s++)
      if (!ws->slice_ev[s] && hipEventCreateWithFlags(&ws->slice_ev[s], hipEventDisableTiming) != hipSuccess) return 1;
    if (form == kUrlStaggered && k > 1) {
      if (!ws->fork2) (void)hipEventCreateWithFlags(&ws->fork2, hipEventDisableTiming);
      if (ws->fork2) ust2 = e->take_stream();
    }
    return k;
  }
  void close() {
    if (ust) e->give_stream(ust);
    if (ust2) e->give_stream(ust2);
    ust = ust2 = nullptr;
  }
};

// TEMPLATE and SIZE in one call: the spans pass rides in url_copy_kernel (one
// walk over the spans)
// (S: the call's slices, each with a grid and a range of the partials of its own)
void fuse_size_into_copy(UrlKernelArgs& ua, SizeKernelArgs& sa, Workspace* ws, size_t size_off, const ose_columns* c,
                         const UrlSlices* S = nullptr) {
  sa.kept_partials = size_partials_of(ws, size_off, c->n_scopes, c->n_resources);
  sa.n_kept_partials = S ? S->part[S->k] : url_copy_blocks(ua.n_groups);
  ua.fuse_size = 1;
  ua.size_partials = const_cast<uint32_t*>(sa.kept_partials);
  ua.sz = sa;
}
}  // namespace

// Workspace layout, one reservation for every stage of the call (a stage
// must not reallocate scratch an earlier stage of the same call is still
// using on the stream):
//   [0, 256)  SAMPLE's words (the OSE_GROUP_BATCH decision SIZE reads);
//             its whole scratch while its slow path may still be queued
//   url_off   the URL stage's scratch
//   size_off  the size stage's sums (after the URL scratch: with TEMPLATE
//             its spans pass runs inside url_copy_kernel)
// The size scratch's per-scope sums are cleared by prepare_size, after the
// join.  With the URL front forked nothing queued earlier touches the bytes
// from size_off on (url_off lies past the whole trace scratch, size_off
// past the URL scratch), so the clear could be queued ahead of the trace
// stage; measured, that fill is starved beside url_plan_kernel (218 us
// instead of 27), delays trace_eval_kernel behind it and costs the C4
// step 0.06 ms (profiles/tail_parts_ab.txt).  Everywhere else the size
// scratch overlaps an earlier stage's (SAMPLE | SIZE: size_off = 256).
StageOffsets stage_offsets(uint32_t mask, bool defer, uint64_t n, uint64_t n_scopes, uint64_t n_resources,
                           uint64_t arena_bytes, uint32_t url_words) {
  const bool sample = mask & OSE_STAGE_SAMPLE;
  StageOffsets s{};
  s.need = sample ? sampling_scratch_bytes(n) : 0;
  s.url_off = sample ? up(defer ? s.need : 256) : 0;
  s.size_off = sample ? 256 : 0;
  if (mask & OSE_STAGE_TEMPLATE) {
    const size_t url_end = s.url_off + url_workspace_bytes(n, arena_bytes, url_words);
    s.need = std::max(s.need, url_end);
    s.size_off = up(url_end);
  }
  if (mask & OSE_STAGE_SIZE) s.need = std::max(s.need, s.size_off + size_scratch_bytes(n_scopes, n_resources));
  return s;
}

// the workspace of a call running every configured stage (SAMPLE's scratch,
// the URL scratch after it, the size sums after that; scopes and resources
// bounded by the spans), a multiple of 256
size_t Engine::workspace_bytes(uint64_t n_spans, uint64_t arena_bytes) const {
  const uint32_t mask = (has_sampling ? OSE_STAGE_SAMPLE : 0) | (has_url ? OSE_STAGE_TEMPLATE : 0) |
                        (has_traffic ? OSE_STAGE_SIZE : 0);
  // (SAMPLE and SIZE without TEMPLATE: a call lays the size sums over the
  // trace scratch, size_off = 256; ose_reserve's size keeps room for them
  // behind it)
  if (has_sampling && has_traffic && !has_url) return sampling_scratch_bytes(n_spans) + size_scratch_bytes(n_spans, n_spans);
  return up(stage_offsets(mask, true, n_spans, n_spans, n_spans, arena_bytes, url_words()).need);
}

int run_stages(Engine* e, const ose_columns* c, const ose_outputs* o, uint32_t mask, uint32_t group_mode,
               const ose_rand* rnd, hipStream_t st) {
  if (!c || !o) return fail(OSE_EINVAL, "columns and outputs are required");
  if (const int mrc = check_stage_mask(e, c, o, mask)) return mrc;
  // SIZE after SQLOP (in this call or an earlier one): the spans pass is
  // sqlop_size_span_kernel, never the one fused into url_copy_kernel
  const bool sql_size = (mask & OSE_STAGE_SIZE) && (mask & (OSE_STAGE_SQLOP | OSE_STAGE_APPLY_SQLOP));
  if (sql_size)
    if (const int src = check_sqlop_size(c, o)) return src;
  // SAMPLE + TEMPLATE by trace id: the URL stage reads nothing SAMPLE writes,
  // so its launches are queued between SAMPLE's fast path and the rest of
  // SAMPLE, which is queued once the host has read the fast path's dup flag
  // (by then the GPU is busy with the URL kernels, and the ~12 gated
  // slow-path launches are skipped when no trace id repeats)
  // SAMPLE without TEMPLATE: the host waits for the fast path right away (an
  // idle gap of one launch latency instead of ~12 gated launches)
  // Inside a hipGraph capture the host can neither wait nor decide: the
  // trace-id stage keeps host state per call (table generations), so it is
  // refused there; every other stage is captured as plain launches.
  const bool capturing = stream_capturing(st);
  if (capturing && (mask & OSE_STAGE_SAMPLE) && group_mode == OSE_GROUP_TRACE_ID)
    return fail(OSE_ENOTSUP, "SAMPLE with OSE_GROUP_TRACE_ID cannot be captured into a hipGraph "
                             "(its trace-id tables advance a host-side generation per call)");
  Workspace* ws = e->acquire_ws(st);
  const uint64_t n = c->n_spans;
  const bool gate_on_host = (mask & OSE_STAGE_SAMPLE) && group_mode == OSE_GROUP_TRACE_ID && n > 0 && !capturing &&
                            !(OSE_DIAG && getenv("OSE_NO_DEFER_SLOW"));
  const bool defer = gate_on_host && (mask & OSE_STAGE_TEMPLATE);
  const StageOffsets so = stage_offsets(mask, defer, n, c->n_scopes, c->n_resources, c->arena_bytes, e->url_words());
  int rc = ws->reserve(so.need);
  const bool tmpl = !rc && (mask & OSE_STAGE_TEMPLATE);
  const bool fused_size_ok = !sql_size && !(OSE_DIAG && getenv("OSE_NO_FUSED_SIZE"));
  std::function<int()> sample_tail;
  UrlKernelArgs ua{};
  // SAMPLE + TEMPLATE (deferred slow path: the URL scratch lies past the
  // trace stage's): the URL planning kernels (plan, slow plan, scan) need
  // nothing from SAMPLE, so they run on a second stream beside the trace
  // stage; the two are latency-bound at four waves per SIMD each and fit a
  // CU together (LDS 2 x 39.7 + 2 x 29.7 KB).  The copy / size launches that
  // read the final keep bytes wait for both.
  UrlFork fork{e, ws, st};
  static const bool one_stream = getenv("OSE_ONE_STREAM") != nullptr;   // per-kernel profiling: no overlap
  // (a small batch's kernels are launch-bound: a fork only adds two events
  // and a stream hand-off to each call of a request-sized batch)
  constexpr uint64_t kForkSpans = 1u << 20;
  // the refs form with the fused spans pass, the one that can run in slices
  // (below); "url_tail_slices" forces the fork for it at any span count
  const bool refs_fused = tmpl && (mask & OSE_STAGE_TEMPLATE_REFS) && (mask & OSE_STAGE_SIZE) && fused_size_ok;
  const uint32_t forced_k = e->url_tail_slices_opt.load(std::memory_order_relaxed);
  const uint32_t plan_groups = (uint32_t)((n + kUrlGroup - 1) / kUrlGroup);
  // (not on the NFA route: no url_plan_kernel)
  const uint32_t want_slices = refs_fused && !e->url_words() ? (forced_k ? forced_k : url_tail_slices(plan_groups)) : 1u;
  const bool forks = !one_stream && !rc && defer && (n >= kForkSpans || (forced_k && refs_fused && !e->url_words()));
  if (forks && want_slices > 1) rc = clear_url_slice_words(e, c, ws, so.url_off, st);
  if (forks && !rc) fork.open();
  ws->beside_url = fork.ust && tmpl;
  // refs form with the fused spans pass: the copy / size launches need only
  // what url_plan_kernel and url_plan_slow_kernel wrote, so the join event is
  // recorded behind those two and url_scan_kernel / url_emit_slow_kernel run
  // on the side stream beside url_copy_kernel / size_tail_kernel; the side
  // stream is joined a second time at the end of the call
#ifndef OSE_URL_JOIN_LATE
  // (not with sql_size: its spans pass reads the refs url_emit_slow_kernel writes)
  fork.early_join = fork.ust && refs_fused;
#endif
  // the plan grid beside the trace stage: 16x the resident workgroups
  // (C4 7.80 -> 7.62 ms, C5 3.49 -> 3.26; 4x: 7.88 / 3.27; alone, C2, the
  // resident grid stays: 16x there is 0.64 -> 2.0 ms, profiles/r5g_plan_grid_ab.txt)
  // The plan grid (refs form): more workgroups than fit at once, so the
  // dispatcher balances the groups' uneven cost (a persistent grid's waves
  // each take a fixed 1/4096 of the groups and the last ones finish late)
  // and, beside the trace stage, interleaves the two kernels' workgroups; a
  // wave's start costs about what a few groups do, so each wave keeps ~19
  // groups: serialised, C4 url_plan 4.30 (resident grid) -> 4.09 (2x) ->
  // 3.92 (4x) -> 3.82 (8x) -> 3.80 ms (16x, the multiplier this rule gives
  // it), C2 0.531 -> 0.520 (2x, its rule) -> 0.542 (4x) -> 0.935 (8x) -> 1.90
  // (16x) (profiles/r6s_plan_grid_serial_ab.txt)
  UrlRun ur;
  ur.ws_off = so.url_off;
  ur.refs = (mask & OSE_STAGE_TEMPLATE_REFS) != 0;
  ur.grid_mult = url_plan_grid_mult(plan_groups, fork.ust != nullptr);
  ur.planned = fork.early_join ? ws->join : nullptr;
  // ... and in slices (kernels.hpp UrlSlices): the spans pass of a slice needs
  // only that slice's plan and the final keep bytes, which the trace stage
  // has written long before the plan ends, so it runs on the caller's stream
  // slice by slice beside the planning of the later slices; only the last
  // slice's pass is left behind the plan.
  const uint32_t form_opt = e->url_tail_form_opt.load(std::memory_order_relaxed);
  const uint32_t form = form_opt ? form_opt - 1 : kUrlTailForm;
  const uint32_t slices = fork.early_join && want_slices > 1 ? fork.open_slices(want_slices, form) : 1u;
  ur.slices = slices;
  ur.form = form;
  ur.slice_ev = ws->slice_ev;
  ur.st2 = fork.ust2;
  ur.fork2 = ws->fork2;
  if (fork.ust && tmpl) {
    rc = run_url(e, c, o, fork.ust, ws, ur, &ua);
    // (an error before the record leaves the join to the usual place)
    fork.join_recorded = fork.early_join && !rc;
  }
  // gateway pipeline order: odigossampling (-24) before odigosurltemplate (1)
  if (!rc && (mask & OSE_STAGE_SAMPLE)) rc = run_sampling(e, c, o, group_mode, rnd, st, ws, gate_on_host ? &sample_tail : nullptr);
  if (sample_tail && !defer) {
    rc = sample_tail();
    sample_tail = nullptr;
  }
  if (!fork.ust && tmpl && !rc) rc = run_url(e, c, o, st, ws, ur, &ua);
  if (sample_tail) {
    const int trc = sample_tail();   // always drained: the host event wait must not be skipped
    if (!rc) rc = trc;
  }
  // join: everything below runs on the caller's stream after both (a sliced
  // call joins slice by slice, below)
  const bool sliced = slices > 1 && fork.join_recorded;
  if (fork.ust2 && !sliced) (void)hipStreamSynchronize(fork.ust2);   // run_url failed between the slices
  if (fork.ust && !sliced) fork.join(ws->join, fork.join_recorded, rc);
  // odigossqldboperationprocessor (orderHint 150): after odigosurltemplate,
  // before odigostrafficmetrics; it reads nothing the earlier stages write
  if (!rc && (mask & OSE_STAGE_SQLOP)) rc = run_sqlop(e, c, o, st);
  // odigostrafficmetrics runs last, on what the earlier stages left (the
  // decisions are final here: SAMPLE's tail has been queued)
  SizeKernelArgs sa{};
  bool size_on = false;
  if (!rc && (mask & OSE_STAGE_SIZE)) rc = prepare_size(e, c, o, mask, group_mode, rnd, st, ws, so.size_off, sa, size_on);
  if (sliced) {
    // (the scope-sum clear of prepare_size thereby runs between the trace
    // stage and the first slice's pass, off the step's tail)
    const UrlSlices S = url_slices(ua.n_groups, slices, form);
    if (!rc && size_on && n > 0) fuse_size_into_copy(ua, sa, ws, so.size_off, c, &S);
    for (uint32_t s = 0; s < S.k; s++) {
      if (S.g[s] == S.g[s + 1]) continue;
      fork.join(ws->slice_ev[s], true, rc);   // every slice is waited for, whatever rc holds
      if (!rc) rc = run_url_back_slice(e, ua, S, s, st);
    }
  } else if (!rc && tmpl) {
    if (size_on && n > 0 && fused_size_ok) fuse_size_into_copy(ua, sa, ws, so.size_off, c);
    rc = run_url_back(e, ua, st);
  }
  if (!rc && size_on) rc = sql_size ? run_sqlop_size_tail(e, sa, o->sql_op, st) : run_size_tail(e, sa, st);
  // second join: the side stream's scan and slow emit end before the
  // caller's stream goes on, the workspace is released and the side
  // stream is handed back
  if (fork.join_recorded) fork.join(ws->join2, false, rc);
  fork.close();
  ws->beside_url = false;
  e->release_ws(ws, st);
  return rc;
}

}  // namespace ose

using namespace ose;

extern "C" {

const char* ose_last_error(void) { return g_last_error.c_str(); }

uint64_t ose_dropped_errors(char* last, size_t cap) {
  std::lock_guard<std::mutex> g(g_dropped_mu);
  if (last && cap) snprintf(last, cap, "%s", g_dropped_last.c_str());
  return g_dropped_count;
}

// Diagnostic, no device: stage_offsets as run_stages calls it (out[0..2] =
// url_off, size_off, need), and out[3] = Engine::workspace_bytes of an engine
// with the mask's stages configured and url_words NFA state words.
extern "C" void osehost_stage_offsets(uint32_t mask, int defer, uint64_t n_spans, uint64_t n_scopes, uint64_t n_resources,
                                      uint64_t arena_bytes, uint32_t url_words, uint64_t* out) {
  const StageOffsets so = stage_offsets(mask, defer != 0, n_spans, n_scopes, n_resources, arena_bytes, url_words);
  Engine e;
  e.has_sampling = mask & OSE_STAGE_SAMPLE;
  e.has_url = mask & OSE_STAGE_TEMPLATE;
  e.has_traffic = mask & OSE_STAGE_SIZE;
  e.url_nfa_words = url_words;
  out[0] = so.url_off;
  out[1] = so.size_off;
  out[2] = so.need;
  out[3] = e.workspace_bytes(n_spans, arena_bytes);
}

int ose_engine_create(const char* cfg_json, ose_engine** out) {
  if (!out) return fail(OSE_EINVAL, "out is NULL");
  *out = nullptr;
  Json root;
  try {
    root = parse_json(cfg_json ? cfg_json : "{}");
  } catch (const std::exception& ex) {
    return fail(OSE_EINVAL, ex.what());
  }
  if (!root.is_obj()) return fail(OSE_EINVAL, "config must be a JSON object");
  auto* e = new Engine();
  std::string err;
  if (const Json* j = root.get("odigosurltemplate")) {
    err = decode_url_config(*j, e->url);
    if (!err.empty()) { delete e; return fail(OSE_EINVAL, err); }
    e->has_url = true;
    e->url_needs_resource = e->url.include.has_value() || e->url.exclude.has_value();
  }
  if (const Json* j = root.get("odigossampling")) {
    err = decode_sampling_config(*j, e->sampling);
    if (!err.empty()) { delete e; return fail(OSE_EINVAL, err); }
    e->has_sampling = true;
  }
  if (const Json* j = root.get("odigostrafficmetrics")) {
    err = decode_traffic_config(*j, e->traffic);
    if (!err.empty()) { delete e; return fail(OSE_EINVAL, err); }
    e->has_traffic = true;
    // newThroughputMeasurementProcessor (processor.go:31-36)
    e->inverse = e->traffic.sampling_ratio != 0 ? (int64_t)(1.0 / e->traffic.sampling_ratio) : 0;
  }
  if (const Json* j = root.get("odigossqldboperationprocessor")) {
    err = decode_sqlop_config(*j, e->sqlop);
    if (!err.empty()) { delete e; return fail(OSE_EINVAL, err); }
    e->has_sqlop = true;
  }
  if (const Json* j = root.get("odigosconditionalattributes")) {
    err = decode_condattr_config(*j, e->condattr);
    if (!err.empty()) { delete e; return fail(OSE_EINVAL, err); }
    if (const int crc = compile_condattr(e->condattr, e->condattr_tab)) { delete e; return crc; }
    e->has_condattr = true;
  }
  if (e->has_url) {
    int rc = build_url_blob(e->url, e->url_blob_host, e->max_name, false, e->url_nfa_words);
    if (rc) { delete e; return rc; }
  }
  int rc = e->build_sampling_tables();
  if (rc) { delete e; return rc; }
  rc = e->build_attr_tables();
  if (rc) { delete e; return rc; }
  rc = ensure_device();
  if (rc) { delete e; return rc; }
  if (hipGetDevice(&e->device) != hipSuccess) { delete e; return fail(OSE_EDEVICE, "hipGetDevice failed"); }
  if (e->has_url) {
    rc = upload(e->url_blob_host, &e->url_blob_dev);
    if (rc) { delete e; return rc; }
  }
  rc = e->upload_sampling_tables();
  if (rc) { delete e; return rc; }
  if (e->has_condattr) {
    rc = upload(e->condattr_tab.blob, &e->condattr_blob_dev);
    if (rc) { delete e; return rc; }
  }
  if (!e->attr_blob_host.empty()) {
    rc = upload(e->attr_blob_host, &e->attr_blob_dev);
    if (rc) { delete e; return rc; }
    std::vector<uint8_t> hm(8 * std::max<size_t>(e->attr_words, 1), 0);
    std::memcpy(hm.data(), e->attr_host_words.data(), 8 * std::min<size_t>(e->attr_host_words.size(), e->attr_words));
    rc = upload(hm, &e->attr_host_mask_dev);
    if (rc) { delete e; return rc; }
  }
  {
    hipError_t he = hipMalloc(reinterpret_cast<void**>(&e->path_count_dev), 64);
    if (he == hipSuccess) he = hipMemset(e->path_count_dev, 0, 64);
    if (he != hipSuccess) {
      delete e;
      return fail(OSE_EDEVICE, std::string("path counters: ") + hipGetErrorString(he));
    }
  }
  *out = reinterpret_cast<ose_engine*>(e);
  return 0;
}

uint32_t ose_engine_path_counts(ose_engine* eng, uint64_t* counts, uint32_t cap) {
  if (!eng) return 0;
  Engine* e = reinterpret_cast<Engine*>(eng);
  uint64_t c[5] = {0, 0, 0, 0, 0};
  if (e->path_count_dev && bind_device(e) == 0) {
    LastErrorScope keep("ose_engine_path_counts");
    // counters the queued work has not reached yet are not counted: the
    // device is synchronised first
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(c, e->path_count_dev, 32, hipMemcpyDeviceToHost) != hipSuccess)
      c[0] = c[1] = c[2] = c[3] = 0;
  }
  // device words 2 and 3 (the URL stage's lists, "url_path_counts") are counts[3] and [4]
  c[4] = c[3];
  c[3] = c[2];
  c[2] = e->long_run_passes.load();
  for (uint32_t k = 0; k < 5 && k < cap && counts; k++) counts[k] = c[k];
  return 5;
}

uint64_t ose_engine_url_nfa_groups(ose_engine* eng) {
  if (!eng) return 0;
  Engine* e = reinterpret_cast<Engine*>(eng);
  uint64_t c = 0;
  if (e->path_count_dev && bind_device(e) == 0) {
    LastErrorScope keep("ose_engine_url_nfa_groups");
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&c, e->path_count_dev + 4, 8, hipMemcpyDeviceToHost) != hipSuccess)
      c = 0;
  }
  return c;
}

void ose_engine_destroy(ose_engine* eng) {
  if (!eng) return;
  Engine* e = reinterpret_cast<Engine*>(eng);
  e->closed.store(true);
  engine_unref(e);
}

int ose_host_alloc(size_t bytes, void** out) {
  if (!out) return fail(OSE_EINVAL, "NULL argument");
  int rc = ensure_device();
  if (rc) return rc;
  HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return 0;
}
void ose_host_free(void* p) {
  LastErrorScope keep("ose_host_free");
  if (p) (void)hipHostFree(p);
}

int ose_set_device(int device) {
  int rc = ensure_device();
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  return 0;
}

uint32_t ose_engine_service_id(const ose_engine* eng, const char* name, size_t len) {
  if (!eng || !name) return OSE_NONE;
  const Engine* e = reinterpret_cast<const Engine*>(eng);
  auto it = e->service_ids.find(std::string(name, len));
  return it == e->service_ids.end() ? OSE_NONE : it->second;
}

int ose_engine_get_info(const ose_engine* eng, ose_engine_info* info) {
  if (!eng || !info) return fail(OSE_EINVAL, "NULL argument");
  const Engine* e = reinterpret_cast<const Engine*>(eng);
  info->stages = (e->has_sampling ? OSE_STAGE_SAMPLE : 0) | (e->has_url ? OSE_STAGE_TEMPLATE : 0) |
                 (e->has_traffic ? OSE_STAGE_SIZE : 0) | (e->has_sqlop ? OSE_STAGE_SQLOP : 0) |
                 (e->has_condattr ? OSE_STAGE_CONDATTR : 0);
  info->max_template_name = e->max_name;
  info->inverse_sampling = e->inverse;
  info->traffic_sampling_ratio = e->traffic.sampling_ratio;
  info->n_attr_rules = e->attr_n_rules;
  info->n_attr_keys = (uint32_t)e->attr_keys.size();
  info->attr_host_rules = e->attr_host_rules;
  return 0;
}

uint32_t ose_engine_attr_host_rules(const ose_engine* eng, uint64_t* words, uint32_t cap) {
  if (!eng) return 0;
  const Engine* e = reinterpret_cast<const Engine*>(eng);
  if (!e->attr_n_rules) return 0;
  const uint32_t W = e->attr_words;
  for (uint32_t w = 0; w < W && w < cap && words; w++) words[w] = w < e->attr_host_words.size() ? e->attr_host_words[w] : 0;
  return W;
}

int ose_engine_set_option(ose_engine* eng, const char* name, int64_t value) {
  if (!eng || !name) return fail(OSE_EINVAL, "NULL argument");
  Engine* e = reinterpret_cast<Engine*>(eng);
  static const struct { const char* name; uint32_t bit; } kOpts[] = {
      {"otlp_gpu_chain", Engine::kOptOtlpGpuChain},
      {"otlp_host_resources", Engine::kOptOtlpHostResources},
      {"otlp_host_scopes", Engine::kOptOtlpHostScopes},
      {"encode_host", Engine::kOptEncodeHost},
      {"otlp_sqlop", Engine::kOptOtlpSqlop},
      {"url_path_counts", Engine::kOptUrlPathCounts},
      {"otlp_condattr", Engine::kOptOtlpCondattr},
      {"url_regex_nfa", Engine::kOptUrlRegexNfa},
      {"otlp_url_full", Engine::kOptOtlpUrlFull},
  };
  // the two options that carry a number (engine_internal.hpp url_tail_slices_opt)
  if (strcmp(name, "url_tail_slices") == 0) {
    if (value < 0 || value > (int64_t)kUrlMaxSlices) return fail(OSE_EINVAL, "engine option url_tail_slices: 0 to 8");
    e->url_tail_slices_opt.store((uint32_t)value);
    return 0;
  }
  if (strcmp(name, "url_tail_form") == 0) {
    if (value < 0 || value > 2) return fail(OSE_EINVAL, "engine option url_tail_form: 0 (the rule), 1 in order, 2 staggered");
    e->url_tail_form_opt.store((uint32_t)value);
    return 0;
  }
  for (const auto& o : kOpts) {
    if (strcmp(name, o.name) != 0) continue;
    if (o.bit == Engine::kOptOtlpSqlop && !e->has_sqlop)
      return fail(OSE_EINVAL, "engine option otlp_sqlop: odigossqldboperationprocessor is not configured");
    if (o.bit == Engine::kOptOtlpUrlFull && !e->has_url)
      return fail(OSE_EINVAL, "engine option otlp_url_full: odigosurltemplate is not configured");
    if (o.bit == Engine::kOptOtlpCondattr) {
      if (!e->has_condattr)
        return fail(OSE_EINVAL, "engine option otlp_condattr: odigosconditionalattributes is not configured");
      if (value)
        if (const int rc = build_condattr_keytab(e)) return rc;
    }
    if (o.bit == Engine::kOptUrlRegexNfa) {
      if (!e->has_url) return fail(OSE_EINVAL, "engine option url_regex_nfa: odigosurltemplate is not configured");
      if (value && !e->url_blob_forced_dev) {   // built once; off again goes back to the tables of ose_engine_create
        if (int brc = bind_device(e)) return brc;
        std::vector<uint8_t> blob;
        uint32_t max_name = 0, words = 0;
        if (const int rc = build_url_blob(e->url, blob, max_name, true, words)) return rc;
        if (const int rc = upload(blob, &e->url_blob_forced_dev)) return rc;
        e->url_forced_words = words;
      }
    }
    if (value) e->options.fetch_or(o.bit);
    else e->options.fetch_and(~o.bit);
    return 0;
  }
  return fail(OSE_EINVAL, std::string("unknown engine option: ") + name);
}

int ose_reserve(ose_engine* eng, uint64_t n_spans, uint64_t arena_bytes) {
  if (!eng) return fail(OSE_EINVAL, "NULL engine");
  Engine* e = reinterpret_cast<Engine*>(eng);
  if (int brc = bind_device(e)) return brc;
  Workspace* ws = e->acquire_ws(nullptr);
  int rc = ws->reserve(e->workspace_bytes(n_spans, arena_bytes));
  if (!rc && e->has_sampling) rc = ws->reserve_table(n_spans);
  if (!rc && e->attr_n_dev) rc = ws->reserve_attr(n_spans);
  if (!rc && e->sampling_chunks_dev.size() > 1) rc = ws->reserve_fold(std::max<uint64_t>(n_spans, 1));
  e->release_ws(ws, nullptr);
  return rc;
}

int ose_process_device(ose_engine* eng, const ose_columns* cols, const ose_outputs* outs, uint32_t stage_mask,
                       uint32_t group_mode, const ose_rand* rnd, void* hip_stream) {
  if (!eng) return fail(OSE_EINVAL, "NULL engine");
  if (int brc = bind_device(reinterpret_cast<Engine*>(eng))) return brc;
  return run_stages(reinterpret_cast<Engine*>(eng), cols, outs, stage_mask, group_mode, rnd,
                    static_cast<hipStream_t>(hip_stream));
}

int ose_profile_enable(ose_engine* eng, int on) {
  if (!eng) return fail(OSE_EINVAL, "NULL engine");
  reinterpret_cast<Engine*>(eng)->profiling = on != 0;
  return 0;
}

int ose_profile_read(ose_engine* eng, char* json, size_t cap) {
  if (!eng || !json) return fail(OSE_EINVAL, "NULL argument");
  Engine* e = reinterpret_cast<Engine*>(eng);
  if (int brc = bind_device(e)) return brc;
  std::vector<Engine::Timed> ts;
  {
    std::lock_guard<std::mutex> g(e->mu);
    ts.swap(e->timings);
  }
  std::map<std::string, std::pair<uint64_t, double>> acc;
  for (auto& t : ts) {
    HIP_TRY(hipEventSynchronize(t.b));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, t.a, t.b));
    auto& a = acc[t.name];
    a.first++;
    a.second += ms;
  }
  {
    std::lock_guard<std::mutex> g(e->mu);
    for (auto& t : ts) { e->event_pool.push_back(t.a); e->event_pool.push_back(t.b); }
  }
  std::string s = "{";
  for (auto& kv : acc) {
    if (s.size() > 1) s += ",";
    char buf[256];
    snprintf(buf, sizeof buf, "\"%s\":{\"launches\":%llu,\"ms\":%.6f}", kv.first.c_str(),
             (unsigned long long)kv.second.first, kv.second.second);
    s += buf;
  }
  s += "}";
  if (s.size() + 1 > cap) return fail(OSE_ERANGE, "profile buffer too small");
  std::memcpy(json, s.c_str(), s.size() + 1);
  return 0;
}

int ose_device_info(char* buf, size_t cap) {
  if (!buf || cap == 0) return fail(OSE_EINVAL, "NULL buffer");
  int rc = ensure_device();
  if (rc) { snprintf(buf, cap, "no device"); return rc; }
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, 0));
  snprintf(buf, cap, "%s arch=%s CUs=%d HBM=%.1fGB", p.name, p.gcnArchName, p.multiProcessorCount,
           (double)p.totalGlobalMem / 1e9);
  return 0;
}

}  // extern "C"
