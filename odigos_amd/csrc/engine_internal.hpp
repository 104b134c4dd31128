// engine_internal.hpp — the engine object behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/odigos_amd.h"
#include "config.hpp"
#include "condattr_host.hpp"
#include "slab.hpp"
#include "timed_launch.hpp"

namespace ose {

int fail(int code, const std::string& msg);
// a HIP call whose failure ends the enclosing function with OSE_EDEVICE
#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess) return fail(OSE_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)
struct Engine;
// makes the engine's device current on the calling thread (a shim's
// goroutines migrate across OS threads; HIP's current device is per thread)
int bind_device(const Engine* e);
int upload(const std::vector<uint8_t>& host, uint8_t** dev);   // hipMalloc + copy
int ensure_device();
void engine_retain(Engine* e);
// drops one reference; the last one synchronises the device and frees the engine
void engine_unref(Engine* e);
// The release entry points return nothing, so a HIP error their clean-up
// meets cannot be returned; it is taken out of the runtime's per-thread
// last-error slot (where the caller's next launch check, torch's or a
// shim's, would report it against its own work) and recorded instead:
// ose_dropped_errors() gives the count and the last one (the GPU tests fail
// on any).  An error already pending on entry is left alone.
void note_dropped_error(const char* where, hipError_t err);
struct LastErrorScope {
  const char* where;
  hipError_t prev;
  explicit LastErrorScope(const char* w) : where(w), prev(hipPeekAtLastError()) {}
  ~LastErrorScope() {
    if (prev != hipSuccess) return;
    const hipError_t now = hipGetLastError();
    if (now != hipSuccess) note_dropped_error(where, now);
  }
};
bool stream_capturing(hipStream_t st);
struct Engine;
void release_exchange_scratch(const Engine* e);   // shard_host.cpp
void release_batch_pool(Engine* e);                // batch.cpp
struct OtlpEngine;
void release_otlp(Engine* e);                      // otlp_host.cpp
void release_encode(Engine* e);                    // otlp_encode.cpp
void release_condattr(Engine* e);                  // condattr_host.cpp
int build_condattr_keytab(Engine* e);              // condattr_host.cpp (engine option otlp_condattr)

// What the groupbytrace store (gbt_host.cpp) reads of a decoded ose_otlp_batch
// and writes into the one it releases (the type is otlp_batch.hpp's; these
// are otlp_host.cpp's, the encode of a released batch otlp_encode_host.cpp's).
struct OtlpBatchView {
  Engine* e;
  const ose_columns* cols;
  bool released;                 // a store's released batch (not to be added again)
  const uint64_t* d_spans;       // [n_spans] Span payload refs (device)
  // the ResourceSpans / ScopeSpans payload refs: on the device when the GPU
  // walked the ResourceSpans level, else host arrays
  bool res_on_device;
  const uint64_t *d_res_ref, *d_scope_ref;
  const uint64_t *h_res_ref, *h_scope_ref;
  size_t h_res_n, h_scope_n;
};
void otlp_batch_view(const ose_otlp_batch* b, OtlpBatchView* v);
struct OtlpReleasedLayout {      // device arrays, as the GPU encoder reads them
  const uint64_t* spans;
  const uint32_t* span0;
  const uint64_t *hdr, *schema;
  const uint64_t* res_ref;
  const uint32_t* res_scope0;
  const uint64_t* scope_ref;
};
ose_otlp_batch* otlp_released_new(Engine* e);      // holds no engine reference: the store does
void otlp_released_delete(ose_otlp_batch* b);
// the released message buffer: at least `bytes`, 256-byte aligned
int otlp_released_arena(ose_otlp_batch* b, size_t bytes, uint8_t** p);
void otlp_released_set(ose_otlp_batch* b, const ose_columns& cols, const OtlpReleasedLayout& lay);

// Device scratch for one in-flight call (look-back status words, sort
// buffers, partial records).  Engines keep a pool so concurrent callers never
// share one.
struct Workspace {
  void* dev = nullptr;
  size_t cap = 0;
  hipEvent_t pending = nullptr;   // recorded at release on the last user's stream
  bool pending_set = false;
  bool captured = false;          // taken by a hipGraph capture: never returned to the pool
  int reserve(size_t bytes);
  // exact trace_id hash table of the SAMPLE stage (trace_slow_kernel.hip table_insert), kept
  // across calls: entries carry a generation tag, so nothing is cleared
  void* table = nullptr;
  uint64_t table_slots_cap = 0;
  uint64_t* dup_bkt = nullptr;         // bucketed duplicate detection (TraceKernelArgs::dup_bkt)
  uint32_t* dup_bkt_count = nullptr;
  uint32_t dup_bkt_bits = 0;
  uint32_t epoch = 0;
  int reserve_table(uint64_t n_spans);
  uint32_t* runs = nullptr;        // run-list path: kMaxRuns run heads per table slot
  uint32_t* run_count = nullptr;
  uint64_t runs_slots = 0;
  int reserve_runs();
  void* fold[2] = {nullptr, nullptr};   // FoldState ping-pong of rule-chunked SAMPLE passes
  uint64_t fold_cap = 0;
  int reserve_fold(uint64_t n_spans);
  uint64_t* attr_bits = nullptr;   // span_attribute bits evaluated on the GPU (attr_host.cpp)
  uint64_t attr_bits_cap = 0;
  int reserve_attr(uint64_t n_spans);
  uint64_t* ep_planes = nullptr;   // endpoint bits per rule chunk of a config with spilled route bytes
  uint64_t ep_planes_cap = 0;      // (words)
  // the caller's columns with the spilled endpoint planes substituted: the
  // SAMPLE stage's host-gated tail reads them after run_sampling returned,
  // so they live with the workspace the call holds, not on its stack
  ose_columns spill_cols{};
  // chunk-local service ids of the resources (Engine::sampling_local_svc):
  // res_svc then res_svc_str, 2 * svc_local_cap words, and the columns that
  // point at them
  uint32_t* svc_local = nullptr;
  uint64_t svc_local_cap = 0;
  ose_columns local_cols{};
  int reserve_svc_local(uint64_t n_resources);
  int reserve_ep_planes(uint64_t words);
  // SAMPLE + TEMPLATE in one call: the fast path's dup flag is copied here and
  // read by the host after the URL launches are queued (run_stages), so the
  // slow-path launches are only queued when a trace id repeats
  uint32_t* dup_host = nullptr;   // pinned
  hipEvent_t dup_ready = nullptr;
  // SAMPLE + TEMPLATE: the URL planning kernels run on a second stream
  // beside the trace stage (run_stages): fork and join events
  hipEvent_t fork = nullptr, join = nullptr, join2 = nullptr;
  // ... planned in slices (kernels.hpp UrlSlices): one event per slice, and
  // the staggered form's second side stream starts behind fork2
  hipEvent_t slice_ev[8] = {};
  hipEvent_t fork2 = nullptr;
  bool beside_url = false;   // this call's trace stage runs beside the forked URL planning
  Workspace() = default;
  Workspace(const Workspace&) = delete;
  ~Workspace();   // frees what it owns (the engine's device is current, nothing in flight)
};

struct Engine {
  // Lifetime: ose_engine_destroy drops the creator's reference; every live
  // child (ose_batch, ose_otlp_batch, ose_otlp_out, ose_gbt) holds one more,
  // so the engine is freed when the last of them is released, in whatever
  // order a shim's finalizers run.  Children released after the destroy are
  // freed instead of pooled.
  std::atomic<int> refs{1};
  std::atomic<bool> closed{false};
  int device = 0;   // the HIP device current when the engine was created; every call runs there
  UrlTemplateConfig url;
  SamplingConfig sampling;
  TrafficMetricsConfig traffic;
  SqlOpConfig sqlop;
  bool has_url = false, has_sampling = false, has_traffic = false, has_sqlop = false;
  // odigosconditionalattributes (condattr_host.cpp): the compiled config, its
  // device copy, and the pinned and device staging of ose_condattr_process
  // (one call at a time: condattr_mu)
  CondAttrConfig condattr;
  bool has_condattr = false;
  CondAttrCompiled condattr_tab;
  uint8_t* condattr_blob_dev = nullptr;
  std::mutex condattr_mu;
  void* condattr_pin = nullptr;
  void* condattr_stage = nullptr;
  size_t condattr_pin_cap = 0, condattr_stage_cap = 0;
  // engine option otlp_condattr: the key table otlp_condattr_kernel looks the
  // span's attribute keys up in (OtlpCaSlot[condattr_slot_mask + 1] on the
  // device), built when the option is first set
  void* condattr_slots_dev = nullptr;
  uint32_t condattr_slot_mask = 0;
  uint64_t condattr_key_lens = 0;
  // ose_engine_set_option: alternative implementations of the OTLP legs
  // (the default path is the fast one; these select the others, for tests
  // that compare the two)
  // kOptOtlpSqlop is a feature switch, not an alternative leg: the OTLP
  // path carries odigossqldboperationprocessor (off until the next ABI version)
  enum : uint32_t {
    kOptOtlpGpuChain = 1, kOptOtlpHostResources = 2, kOptOtlpHostScopes = 4, kOptEncodeHost = 8, kOptOtlpSqlop = 16,
    kOptUrlPathCounts = 32,  // run_url keeps the call's unplanned / slow list lengths (ose_engine_path_counts)
    // a feature switch like kOptOtlpSqlop: the OTLP path carries odigosconditionalattributes
    // (ose_otlp_condattr_columns, ose_otlp_encode_condattr)
    kOptOtlpCondattr = 64,
    // a test and measurement seam: the URL tables rebuilt with every user
    // regexp as an NFA program (url_blob_forced_dev), so a config whose
    // regexps have DFAs runs both routes; set between calls, not during one
    kOptUrlRegexNfa = 128,
    // a feature switch like kOptOtlpSqlop: ose_otlp_decode parses url.full / http.url
    // on the GPU (otlp_url_full_kernel.hip; off until the next ABI version)
    kOptOtlpUrlFull = 256
  };
  std::atomic<uint32_t> options{0};
  bool option(uint32_t o) const { return (options.load(std::memory_order_relaxed) & o) != 0; }
  // "url_tail_slices" (a test and measurement seam): the slices K of the
  // forked refs form's plan and spans pass, forced (and the fork with it, at
  // any span count); 0: url_tail_slices()'s rule.  "url_tail_form": their
  // form + 1 (kernels.hpp kUrlInOrder / kUrlStaggered); 0: the rule's
  std::atomic<uint32_t> url_tail_slices_opt{0}, url_tail_form_opt{0};
  bool url_needs_resource = false;
  int64_t inverse = 1;
  uint32_t max_name = 5;

  std::vector<uint8_t> url_blob_host;
  uint8_t* url_blob_dev = nullptr;
  // state words of the widest NFA program in the URL tables; 0: they hold
  // none and the stage runs as it always did
  uint32_t url_nfa_words = 0;
  // engine option url_regex_nfa: the all-NFA tables, built when first set
  uint8_t* url_blob_forced_dev = nullptr;
  uint32_t url_forced_words = 0;
  bool url_forced() const { return option(kOptUrlRegexNfa) && url_blob_forced_dev; }
  uint32_t url_words() const { return url_forced() ? url_forced_words : url_nfa_words; }
  std::vector<uint8_t> sampling_blob_host;   // = sampling_chunks_host[0]
  uint8_t* sampling_blob_dev = nullptr;      // = sampling_chunks_dev[0]
  // the rule tables in consecutive chunks of the level-ordered rule list,
  // each within the trace stage's bounds (64 latency bits, 64 service +
  // span_attribute bits, kSampCfgLds bytes); one chunk for most configs
  std::vector<std::vector<uint8_t>> sampling_chunks_host;
  std::vector<uint8_t*> sampling_chunks_dev;
  std::vector<uint8_t> sampling_chunk_attr;   // chunk has span_attribute rules
  // trace-id exchange tables (shard_host.cpp): bit s of sampling_lat_svc =
  // service s has an http_latency rule in some chunk; on the device, the K
  // chunk table pointers then those words (ShardArgs::cfgs, ::lat_svc)
  std::vector<uint32_t> sampling_lat_svc;
  uint8_t* shard_tables_dev = nullptr;
  // which slow paths the trace stage took (ose_engine_path_counts): [0] run
  // lists, [1] the radix sort (device counters), [2] long-run passes (host);
  // device words [2] and [3]: the URL stage's unplanned and slow list lengths
  // of the most recent TEMPLATE call ("url_path_counts")
  unsigned long long* path_count_dev = nullptr;
  std::atomic<uint64_t> long_run_passes{0};
  std::unordered_map<std::string, uint32_t> service_ids;
  uint32_t sampling_n_lat = 0, sampling_n_attr = 0;
  uint32_t sampling_n_lat_svc = 0;   // services with http_latency rules (trace_multi_kernel takes <= 64)
  bool sampling_walk_ok = false;     // every chunk has <= 128 rules (SampWalkDev, trace_multi_kernel)
  // a chunk table past kSampCfgLds (a route longer than the LDS table): the
  // trace stage and the pack then take every chunk's endpoint bits as
  // precomputed planes (spill_endpoint_planes)
  bool sampling_spill = false;
  // more interned services than one chunk's dense service tables (12 B per
  // service) fit beside its rules in the LDS budget: each chunk's tables then
  // index chunk-local ids (the services its rules name, n_services of its
  // SampCfgDev), and the trace stage translates the resources' service ids
  // for each chunk's pass (svc_translate_kernel; the trace kernels are
  // unchanged).  Map: [chunk][global id] -> local id or 0xFFFFFFFF.
  bool sampling_local_svc = false;
  std::vector<std::vector<uint32_t>> sampling_svc_map_host;
  std::vector<uint32_t*> sampling_svc_map_dev;
  uint32_t** sampling_svc_maps_dev = nullptr;   // the K map pointers on the device (ShardArgs / OwnerArgs::svc_maps)
  // span_attribute rules: all of them (attr_n_rules), the GPU-evaluated ones
  // (attr_n_dev, attr_kernel.hip) and the keys those read
  std::vector<uint8_t> attr_blob_host;
  uint8_t* attr_blob_dev = nullptr;
  uint32_t attr_n_rules = 0, attr_n_dev = 0;
  uint64_t attr_host_rules = 0;              // rules 0..63 of attr_host_words (ose_engine_info)
  std::vector<uint64_t> attr_host_words;     // the shim-evaluated rules, one bit per rule
  uint32_t attr_words = 1;                   // attr_match words per span: (attr_n_rules + 63) / 64, >= 1
  uint8_t* attr_host_mask_dev = nullptr;     // attr_host_words on the device (AttrArgs::host_mask)
  bool attr_host_rules_any() const {
    for (uint64_t w : attr_host_words)
      if (w) return true;
    return false;
  }
  std::vector<std::string> attr_keys;

  std::mutex mu;
  std::vector<Workspace*> pool, free_ws;
  std::vector<void*> batch_pool;   // released ose_batch slabs (batch.cpp)
  OtlpEngine* otlp = nullptr;      // OTLP ingest tables, built on first use (otlp_host.cpp)
  std::vector<void*> otlp_pool;    // released ose_otlp_batch objects
  std::vector<void*> enc_pool;     // encoder workspaces of released ose_otlp_out objects
  size_t batch_pool_bytes = 0;

  // ose_profile_*: (kernel name, start, stop) per launch
  bool profiling = false;
  struct Timed { const char* name; hipEvent_t a, b; };
  std::vector<Timed> timings;
  std::vector<hipEvent_t> event_pool;
  // One launch under a profile name: `launch` queues it on st (returning
  // nothing, or an int that ends the step when not 0), then the runtime's
  // launch error is checked.  With profiling on, two pooled events bracket it;
  // a failure hands them back to event_pool before its code is returned.
  template <class F>
  int timed(const char* name, hipStream_t st, F&& launch) {
    return timed_launch(*this, name, st, std::forward<F>(launch));
  }

 private:
  template <class P, class S, class F>
  friend int timed_launch(P& p, const char* name, S st, F&& launch);
  hipEvent_t take_event();
  Timed prof_begin(const char* name, hipStream_t st);
  void prof_end(Timed& t, hipStream_t st);
  void prof_drop(Timed& t);
  int launch_status();

 public:

  ~Engine();
  Workspace* acquire_ws(hipStream_t st);
  void release_ws(Workspace* w, hipStream_t st);
  void return_unused_ws(Workspace* w);
  std::vector<hipStream_t> streams, free_streams;   // ose_process (host batches)
  hipStream_t take_stream();
  void give_stream(hipStream_t s);
  int build_sampling_tables();
  int upload_sampling_tables();   // sampling_host.cpp
  int build_attr_tables();
  size_t workspace_bytes(uint64_t n_spans, uint64_t arena_bytes) const;   // every configured stage
};

// tail != nullptr (OSE_GROUP_TRACE_ID only): queue the fast path, then hand
// back in *tail the rest of the stage (slow path if the fast path saw a
// repeated trace id, per-trace compaction); the caller queues other work on
// the stream first and calls *tail before anything that reads keep
int run_sampling(Engine* e, const ose_columns* c, const ose_outputs* o, uint32_t group_mode, const ose_rand* rnd,
                 hipStream_t st, Workspace* ws, std::function<int()>* tail = nullptr);
// the trace stage's scratch past its 256 bytes of words (sampling_host.cpp)
struct SamplingLayout {
  WsPart win_heads, win_base, wstatus, rec, key, k2, v2, k3, v3, hist, hoff, hstatus, long_runs, long_meta, long_pieces,
      long_part, win_first;
  size_t end;
};
SamplingLayout sampling_layout(uint64_t n_spans);
// For the host seams the layout tests read (osehost_*_layout): a layout
// struct is its WsParts in order, then `end`.  Returns the number of parts.
template <class L>
uint32_t layout_parts(const L& l, uint64_t* off, uint64_t* bytes, uint32_t cap, uint64_t* end) {
  constexpr uint32_t kParts = (sizeof(L) - sizeof(size_t)) / sizeof(WsPart);
  static_assert(sizeof(L) == kParts * sizeof(WsPart) + sizeof(size_t), "WsParts, then end");
  const WsPart* p = reinterpret_cast<const WsPart*>(&l);
  for (uint32_t k = 0; k < kParts && k < cap; k++) {
    if (off) off[k] = p[k].off;
    if (bytes) bytes[k] = p[k].bytes;
  }
  if (end) *end = l.end;
  return kParts;
}
size_t sampling_scratch_bytes(uint64_t n_spans);   // = sampling_layout(n_spans).end
// The passes of the stable LSD radix sort on the keys' low `bits` bits (8-bit
// digits: sort_hist, the scan of the 256 * n_tiles counts into hoff,
// sort_scatter), ping-pong between kb[] / vb[].  `s`: n_spans, n_tiles, gate,
// key, error and the scan words set; the first pass reads keys_in / vals_in
// (null: s.key and the identity).  *keys / *vals: the last pass's output.
struct TraceSortArgs;
int radix_passes(TraceSortArgs s, uint32_t* const kb[2], uint32_t* const vb[2], uint32_t* hist, uint32_t* hoff,
                 uint32_t htiles, int bits, const uint32_t* keys_in, const uint32_t* vals_in, hipStream_t st,
                 const uint32_t** keys, const uint32_t** vals);
// every column of `src` (device) whose pointer in `dst` is not NULL, copied there (engine.cpp)
int download_columns(const ose_columns& src, const ose_columns* dst);
// the attr_match bits the trace stage reads for this call (attr_host.cpp)
int resolve_attr_match(Engine* e, const ose_columns* c, Workspace* ws, hipStream_t st, const uint64_t** out);
// size stage scratch at workspace byte `off` (size_host.cpp)
int run_size(Engine* e, const ose_columns* c, const ose_outputs* o, uint32_t mask, uint32_t group_mode,
             const ose_rand* rnd, hipStream_t st, Workspace* ws, size_t off);
struct SizeKernelArgs;
int prepare_size(Engine* e, const ose_columns* c, const ose_outputs* o, uint32_t mask, uint32_t group_mode,
                 const ose_rand* rnd, hipStream_t st, Workspace* ws, size_t off, SizeKernelArgs& a, bool& active);
uint32_t* size_partials_of(Workspace* ws, size_t off, uint64_t n_scopes, uint64_t n_resources);
uint32_t size_partials_cap();   // the kept partials the size scratch reserves (any slicing of the spans pass)
int run_size_tail(Engine* e, const SizeKernelArgs& a, hipStream_t st);
int run_size_scopes(Engine* e, const SizeKernelArgs& a, hipStream_t st);   // size_tail_kernel, size_fix_kernel
size_t size_scratch_bytes(uint64_t n_scopes, uint64_t n_resources);
// odigossqldboperationprocessor (sqlop_host.cpp): the SQLOP launch, the
// columns SIZE needs after it, and run_size_tail with the spans pass that
// counts what sql_op adds
int run_sqlop(Engine* e, const ose_columns* c, const ose_outputs* o, hipStream_t st);
int check_sqlop_size(const ose_columns* c, const ose_outputs* o);
int run_sqlop_size_tail(Engine* e, const SizeKernelArgs& a, const uint8_t* sql_op, hipStream_t st);
// odigosconditionalattributes has entry points of its own: the answer of
// every entry point that takes a stage mask holding OSE_STAGE_CONDATTR
int refuse_condattr(const char* entry);
// every rule chunk's endpoint bits of the spans as planes of n words (a
// config with spilled route bytes: Engine::sampling_spill), sampling_host.cpp
int spill_endpoint_planes(Engine* e, const ose_columns* c, Workspace* ws, hipStream_t st, const uint64_t** out);
// Where each stage's scratch starts in the one workspace of a call, and the
// bytes the call reserves (engine.cpp; the layout is described there)
struct StageOffsets { size_t url_off, size_off, need; };
StageOffsets stage_offsets(uint32_t mask, bool defer, uint64_t n_spans, uint64_t n_scopes, uint64_t n_resources,
                           uint64_t arena_bytes, uint32_t url_words);
int run_stages(Engine* e, const ose_columns* c, const ose_outputs* o, uint32_t mask, uint32_t group_mode,
               const ose_rand* rnd, hipStream_t st);
// odigosurltemplate (url_host.cpp): the table compiler, the stage's workspace
// and its launches in two halves
int build_url_blob(const UrlTemplateConfig& c, std::vector<uint8_t>& out, uint32_t& max_name, bool force_nfa,
                   uint32_t& nfa_words);
struct UrlLayout {
  // the words one memset clears: [0] scan counter, [4] slow count, [8] error,
  // [12] unplanned count, then the refs form's bump and aligned slow sum, then
  // the scan status (8 bytes per scan tile)
  WsPart zero, bump, slow_aligned, scan_status;
  WsPart len, meta, code, gsum, gbase, gscr, slow, unpl, dbg;
  WsPart scr;    // the assembled group images (refs form: none, they go to tmpl_arena)
  WsPart slab;   // the NFA route's state slab (no NFA program: none)
  size_t end;
};
UrlLayout url_layout(uint64_t n_spans, uint64_t arena_bytes, uint32_t nfa_words, bool refs);
size_t url_workspace_bytes(uint64_t n_spans, uint64_t arena_bytes, uint32_t nfa_words = 0);   // the non-refs layout's end
struct UrlKernelArgs;
// What run_url takes past the workspace.  ws_off: the URL scratch starts this
// many bytes into the workspace (past a SAMPLE stage's scratch whose slow path
// is still to be queued).  refs: the OSE_STAGE_TEMPLATE_REFS form.  grid_mult:
// url_plan_grid_mult's.  planned: an event recorded on st behind
// url_plan_slow_kernel, when every span's plan_len and url_out are written
// (all the refs form's spans pass reads).
// slices > 1 (kernels.hpp UrlSlices; the forked refs form only): the plan
// launches go slice by slice, slice s's event slice_ev[s] is recorded behind
// its url_plan_slow_kernel instead of `planned`, and in the staggered form
// the odd slices run on st2, which st waits for before the scan.
struct UrlRun {
  size_t ws_off = 0;
  bool refs = false;
  uint32_t grid_mult = 1;
  hipEvent_t planned = nullptr;
  uint32_t slices = 1;
  uint32_t form = 0;
  hipEvent_t* slice_ev = nullptr;   // [slices]
  hipStream_t st2 = nullptr;        // staggered form
  hipEvent_t fork2 = nullptr;       // ... st2 starts behind st's clears
};
struct UrlSlices;
// the front (plan, plan_slow, scan, emit_slow); the arguments of the rest go
// to *front, and run_url_back queues url_copy, fused with
// odigostrafficmetrics' spans pass when front->fuse_size is set
int run_url(Engine* e, const ose_columns* c, const ose_outputs* o, hipStream_t st, Workspace* ws, const UrlRun& r,
            UrlKernelArgs* front);
int run_url_back(Engine* e, const UrlKernelArgs& a, hipStream_t st);
// a sliced call: its count words cleared (on the caller's stream, before the
// fork), the arguments of slice s's launches, and its spans pass
int clear_url_slice_words(Engine* e, const ose_columns* c, Workspace* ws, size_t ws_off, hipStream_t st);
UrlKernelArgs url_slice_args(const UrlKernelArgs& a, const UrlSlices& S, uint32_t s);
int run_url_back_slice(Engine* e, const UrlKernelArgs& a, const UrlSlices& S, uint32_t s, hipStream_t st);

}  // namespace ose
