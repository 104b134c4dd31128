// kernels.hpp — host-side launch interfaces of the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/odigos_amd.h"

// OSE_DIAG=1: the diagnostics build (python -m odigos_amd.build --variant _diag
// OSE_DIAG=1; loaded with OSE_LIB_VARIANT=_diag): ablation switches, per-section
// clocks and tuning knobs read from the environment.  The product library is
// built without it and reads no such variable.
#ifndef OSE_DIAG
#define OSE_DIAG 0
#endif

namespace ose {

// odigosurltemplate: four launches on one stream (url_kernel.hip).
//   url_plan_kernel  one wave per 64-span group: plan, output length per span
//                    and the group's template bytes, assembled in LDS and
//                    stored to the wave's scratch region
//   url_plan_slow_kernel  the groups the plan kernel could not plan from its
//                    LDS stage (byte range over the stage, segment list
//                    overflow, a segment over 64 bytes): planned per span from HBM
//   url_scan_kernel  exclusive scan of the per-group output sums
//   url_copy_kernel  one wave per group: template refs, and the group's bytes
//                    copied from scratch to their place in the output arena
//   url_emit_slow_kernel  the groups the plan kernel could not assemble (user
//                    rules, oversized groups), from the plan arrays
struct SizePart {            // one resource run's share of a 64-scope window
  uint32_t r;                 // the resource
  uint32_t ch;                // alive scopes (bits 0-29) | had spans << 30 | whole side << 31
  uint64_t v;                 // framed scope bytes
};
struct SizeKernelArgs {
  uint64_t n_spans;
  uint32_t n_scopes, n_resources, n_attrsets;
  uint32_t sampled;           // SAMPLE ran in this call: keep decides which spans survive
  uint32_t templated;         // TEMPLATE ran: url_out / tmpl grow the spans
  uint32_t remove_empty;      // OSE_GROUP_TRACE_ID sampling: emptied scopes/resources are removed
  const uint32_t* batch_keep; // OSE_GROUP_BATCH sampling: 0 empties the whole call (null otherwise)
  const uint32_t* span_size;
  const uint32_t* name_len;
  const uint32_t* scope;
  const uint32_t* scope_size;
  const uint32_t* scope_resource;
  const uint32_t* res_size;
  const uint32_t* res_attrset;
  const uint8_t* keep;
  const uint8_t* url_out;
  const uint8_t* kind;
  const ose_strref* tmpl;
  int64_t inverse;
  uint64_t* scope_body;       // [S] zeroed: body bytes | runs that added << kSumBits (size_device.hpp)
  // the fused scopes + resources pass (size_tail_kernel): per 64-scope window
  // its first and last resource run's partial sums, and whether the window
  // holds the end of a run that began in an earlier window (size_fix_kernel)
  SizePart* parts;            // [2 * n_swin], written every call
  uint32_t* fix;              // [n_swin], written every call
  uint32_t n_swin;            // ceil(n_scopes / 64)
  int64_t* attrset_bytes;     // [n_attrsets] added to
  int64_t* accepted;          // [1] added to
  uint64_t* res_bytes;        // [R] or null
  // the spans pass ran fused in url_copy_kernel: the surviving spans counted
  // per block there, summed by size_tail_kernel (null: size_span_kernel counted)
  const uint32_t* kept_partials;
  uint32_t n_kept_partials;
};

struct UrlKernelArgs {
  uint64_t n_spans;
  // The groups url_plan_kernel, url_plan_slow_kernel and the refs instance of
  // url_copy_kernel work on in this launch: [0, n_groups), or one slice of it
  // (UrlSlices; run_stages).  (Here, beside n_spans: one scalar load brings
  // all the plan kernel's loop bounds.)
  uint32_t g_begin, g_end;
  const uint8_t* arena;
  const uint8_t* url_flags;
  const uint8_t* kind;
  const uint32_t* resource;
  const uint8_t* res_url_ok;   // may be null (no include/exclude)
  const ose_strref* path;
  uint8_t* url_out;
  ose_strref* tmpl;
  uint8_t* out_arena;
  uint64_t out_cap;
  const uint8_t* cfg;          // UrlCfgDev blob
  // workspace
  uint32_t* plan_len;          // [n_spans] output length
  uint32_t* plan_meta;         // [n_spans] mode/lead/slow/url_out/field (slow groups only)
  uint64_t* plan_code;         // [n_spans] per-segment name ids (slow groups only)
  uint8_t* scratch;            // assembled group images: wave w owns [w * scr_region, +scr_region)
  uint64_t scr_region;         // bytes per wave (multiple of 16)
  uint64_t* group_scr;         // [n_groups] scratch offset of the group's image, ~0: slow group
  uint64_t* group_sum;         // [n_groups]
  uint64_t* group_base;        // [n_groups] exclusive prefix
  uint32_t n_groups;           // ceil(n_spans / kUrlGroup)
  uint32_t n_scan_tiles;       // ceil(n_groups / kUrlScanTile)
  uint32_t* scan_counter;      // zeroed before launch
  uint64_t* scan_status;       // [n_scan_tiles], zeroed before launch
  uint32_t* error;             // bit0 look-back timeout, bit1 output overflow
  uint64_t* used;              // bytes written (optional)
  uint32_t* slow_count;        // groups the plan kernel left to K3s (zeroed before launch)
  uint32_t* slow_groups;       // [n_groups]
  uint32_t* unplanned_count;   // groups the plan kernel left to url_plan_slow_kernel (zeroed before launch)
  uint32_t* unplanned;         // [n_groups]
  uint32_t general;            // user rules or custom ids configured (selects the general kernel instances)
  // the tables hold an NFA program (devcfg.hpp NfaDev): url_plan_kernel is
  // not launched, url_nfa_fill_kernel lists every group and the NFA instances
  // of the slow kernels plan and emit them per lane.  nfa_words: state words
  // of the widest program; nfa_slab: kUrlNfaMaxWaves columns of 2 * nfa_words
  // words per lane, word-major across the wave's lanes (workspace)
  uint32_t nfa, nfa_words;
  uint32_t* nfa_slab;
  // OSE_STAGE_TEMPLATE_REFS: scratch is the caller's tmpl_arena (== out_arena),
  // the fast groups' images stay where url_plan_kernel wrote them (their refs
  // point there, url_copy_kernel copies nothing).  A plan wave takes its
  // image space in chunks of refs_chunk bytes from *bump (zeroed before the
  // launch); the scan places the slow groups from the final *bump on.
  uint32_t refs;
  uint64_t* bump;
  uint64_t refs_chunk;          // url_refs_chunk()
  uint32_t plan_waves;          // url_plan_waves()
  uint64_t* slow_aligned;       // refs: sum of the scan-placed groups' sizes rounded up to 16 (zeroed)
  uint32_t plan_grid_mult;     // refs form beside the trace stage: plan workgroups = resident x this (run_stages)
  uint32_t ablate;             // diagnostics only (OSE_URL_ABLATE): 1 skip emission, 2 skip planning, 4 skip bitmaps
  uint64_t* dbg;               // diagnostics only (ablate & 512): per-section clock sums
  // odigostrafficmetrics' spans pass fused into url_copy_kernel (TEMPLATE and
  // SIZE in one call): sz as size_span_kernel would get it, sz.tmpl unused
  // (the plan lengths are the template lengths); the kept count of block b
  // goes to size_partials[b] (launch_url_copy's grid, <= kUrlCopyMaxBlocks)
  uint32_t fuse_size;
  uint32_t* size_partials;
  SizeKernelArgs sz;
  // A slice's launches ([g_begin, g_end) above) have its own unplanned list
  // and count word (unplanned + g_begin, so the lists never overlap) and add
  // the list lengths into *unplanned_total (null: not sliced); its spans pass
  // runs copy_blocks workgroups (0: url_copy_blocks(n_groups)) and counts
  // into size_partials[partial_off + block].
  uint32_t copy_blocks, partial_off;
  uint32_t* unplanned_total;
};
constexpr uint32_t kUrlCopyMaxBlocks = 65536;
uint32_t url_copy_blocks(uint32_t n_groups);
constexpr uint32_t kUrlGroup = 64;       // spans per wave group (url_kernel.hip kWave)
constexpr uint32_t kUrlScanTile = 1024;  // groups per scan workgroup (url_kernel.hip kScanThreads)
// (the URL stage's workspace for n spans: url_host.cpp url_layout)
constexpr uint32_t kUrlMaxWaves = 4096;  // waves of the persistent plan grid (>= its resident waves)
constexpr uint32_t kUrlWaveSlack = 8192; // scratch bytes per wave on top of its share
// scratch for the assembled group images of a batch whose arena holds
// arena_bytes: the path bytes bound the templates but for inserted names,
// hence 1.25x plus a per-wave slack; a group that does not fit its wave's
// region is emitted by url_emit_slow_kernel instead
inline size_t url_scratch_bytes(uint64_t n, uint64_t arena_bytes) {
  const uint64_t g = (n + kUrlGroup - 1) / kUrlGroup;
  const uint64_t w = g < kUrlMaxWaves ? g : kUrlMaxWaves;
  return ((arena_bytes + n + (arena_bytes + n) / 4 + 15) & ~15ull) + w * kUrlWaveSlack;
}
// the NFA route's state slab: one column of 2 * nfa_words words per lane for
// every wave of the NFA kernels' grids (at most kUrlNfaMaxWaves, and no more
// than the batch has groups, rounded up to a workgroup of four)
constexpr uint32_t kUrlNfaMaxWaves = 1024;
inline uint32_t url_nfa_waves(uint64_t n) {
  const uint64_t g = ((n + kUrlGroup - 1) / kUrlGroup + 3) & ~3ull;
  return (uint32_t)(g < kUrlNfaMaxWaves ? g : kUrlNfaMaxWaves);
}
inline size_t url_nfa_slab_bytes(uint64_t n, uint32_t nfa_words) {
  return nfa_words ? 256 + (size_t)url_nfa_waves(n) * 2 * nfa_words * kUrlGroup * 4 : 0;
}
// refs form: the plan grid in multiples of the resident one, from the batch's
// groups (engine.cpp run_stages); OSE_PLAN_GRID_OLD builds: 16 beside the
// trace stage, 1 otherwise (A/B)
#ifndef OSE_PLAN_GRID_OLD
#define OSE_PLAN_GRID_OLD 0
#endif
inline uint32_t url_plan_grid_mult(uint32_t n_groups, bool forked = false) {
  if (OSE_PLAN_GRID_OLD) return forked ? 16u : 1u;
  const uint32_t m = n_groups / (kUrlMaxWaves * 19u);
  return m < 1 ? 1u : m > 16 ? 16u : m;
}
// The one-GPU forked refs form with the fused spans pass (run_stages) cuts
// the batch's groups into K slices of consecutive groups: each slice is
// planned by its own url_plan_kernel / url_plan_slow_kernel launches on the
// side stream(s), and its spans pass (url_copy_kernel<true, true>) runs on the
// caller's stream as soon as the slice is planned, beside the planning of the
// later slices, instead of behind the whole plan.
//   kUrlInOrder    equal slices, one after another on one side stream
//   kUrlStaggered  slices alternating between two side streams, the first
//                  half as long as the others, so a slice's ramp falls into
//                  the drain of the slice before it
enum : uint32_t { kUrlInOrder = 0, kUrlStaggered = 1 };
constexpr uint32_t kUrlMaxSlices = 8;
// (a first slice of 2/3 or 4/5 of the others measured the same as 1/2 at
// K = 2, 6.69-6.70 ms on C4; with 4/5 the first slice's url_plan_slow_kernel
// ends 0.4 ms late beside the other slice's plan, with 1/2 that is hidden)
constexpr uint32_t kUrlStaggerNum = 1, kUrlStaggerDen = 2;
struct UrlSlices {
  uint32_t k;                          // slices (1: the unsliced call)
  uint32_t g[kUrlMaxSlices + 1];       // slice s holds the groups [g[s], g[s + 1])
  uint32_t part[kUrlMaxSlices + 1];    // ... and its spans pass counts into size_partials[part[s], part[s + 1])
};
// (the spans pass's grid over a slice: the unsliced grid's cap shared among
// the slices, so the K grids together never count into more than
// kUrlCopyMaxBlocks partials, which is what the size scratch reserves, and a
// wave keeps the groups it has in the unsliced grid of a large batch)
inline uint32_t url_slice_copy_blocks(uint32_t groups, uint32_t k) {
  if (k <= 1) return url_copy_blocks(groups);
  const uint32_t want = (groups + 7) / 8, cap = kUrlCopyMaxBlocks / k;
  return groups == 0 ? 0u : want < cap ? want : cap;
}
inline UrlSlices url_slices(uint32_t n_groups, uint32_t k, uint32_t form) {
  UrlSlices s{};
  s.k = k < 1 ? 1u : k > kUrlMaxSlices ? kUrlMaxSlices : k;
  // staggered: the first slice kUrlStaggerNum / kUrlStaggerDen of each other
  // one (bounds rounded up: no slice is empty once there are K groups)
  const uint64_t first = form == kUrlStaggered ? kUrlStaggerNum : 1, each = form == kUrlStaggered ? kUrlStaggerDen : 1;
  const uint64_t d = first + (s.k - 1) * each;
  for (uint32_t j = 1; j < s.k; j++) {
    const uint64_t num = (uint64_t)n_groups * (first + (j - 1) * each);
    s.g[j] = (uint32_t)((num + d - 1) / d);
  }
  s.g[s.k] = n_groups;
  for (uint32_t j = 0; j < s.k; j++) s.part[j + 1] = s.part[j] + url_slice_copy_blocks(s.g[j + 1] - s.g[j], s.k);
  return s;
}
// The slices of a batch of n_groups groups (1: unsliced) and their form
// (profiles/tail_slices_ab.txt, one MI355X, C4).  Every url_plan_kernel
// launch that starts behind another on one stream costs about 0.2 ms (the
// grid drains and refills), more than a slice's spans pass saves: in order,
// 100M spans run 6.82 (K = 1) -> 7.04 (2) -> 7.28 (3) -> 7.45 (4) -> 8.14 ms
// (8).  Staggered, two slices start together and nothing drains before the
// end: 6.69 (2) -> 6.81 (3) -> 6.88 (4) -> 6.92 (8); a third launch again
// costs more than it saves.  Two staggered slices gain 0.13 ms at 100M spans,
// 0.03 at 30M (one run each, inside the noise) and lose 0.05 at 10M and 0.04
// at 3M, so the rule slices from 2^20 groups (67M spans) up.
constexpr uint32_t kUrlTailForm = kUrlStaggered;
constexpr uint32_t kUrlTailGroups = 1u << 20;
inline uint32_t url_tail_slices(uint32_t n_groups) { return n_groups >= kUrlTailGroups ? 2u : 1u; }
void launch_url_plan(const UrlKernelArgs& a, hipStream_t st);
uint32_t url_plan_waves(const UrlKernelArgs& a);   // waves of the plan grid (scratch regions)
// refs form: the image chunk size for an arena of `cap` bytes over `waves`
// plan waves (0: every group image takes exactly its size)
uint64_t url_refs_chunk(uint64_t cap, uint32_t waves);
void launch_url_scan(const UrlKernelArgs& a, hipStream_t st);
void launch_url_copy(const UrlKernelArgs& a, hipStream_t st);
void launch_url_plan_slow(const UrlKernelArgs& a, hipStream_t st);
void launch_url_emit_slow(const UrlKernelArgs& a, hipStream_t st);
// the NFA route (UrlKernelArgs::nfa): the fill kernel in url_plan_kernel's
// place, then the NFA instances of the two slow kernels
void launch_url_nfa_fill(const UrlKernelArgs& a, hipStream_t st);
void launch_url_nfa_plan(const UrlKernelArgs& a, hipStream_t st);
void launch_url_nfa_emit(const UrlKernelArgs& a, hipStream_t st);

}  // namespace ose

namespace ose {

// odigossampling: trace grouping, per-trace reduction and the rule fold
// (trace_kernel.hip; the slow paths: trace_slow_kernel.hip).  A "position" is an index into the evaluation order:
// the batch order itself (fast path) or the stable sort of spans by trace
// (slow path, perm != null).
struct TraceSlot {            // exact trace_id hash table entry (32 B)
  uint32_t state;             // epoch << 2 | {0 empty, 1 busy, 2 ready}
  uint32_t first;             // smallest run-head position of this trace_id
  uint64_t hi, lo;
  uint64_t _pad;
};
struct TraceRec {             // per-trace record, stored at the trace's head position
  uint32_t first_span;
  uint8_t keep, level, _p0, _p1;
  double ratio;
};
enum : uint32_t { kTraceRuns = 0, kTracePerm = 1, kTraceBatch = 2 };
// ShouldSample's walk between the passes of a rule-chunked configuration
// (sampling_host.cpp build_sampling_tables): the level being folded, its
// evaluateLevel accumulators and the min fallback of the closed levels
struct FoldState {
  double ratio;      // the open level's ratio (after kFsDone: the satisfied level's)
  double min_fb;     // min fallback over closed matched levels (kFsHaveMin)
  uint32_t level;    // the open level (after kFsDone: the satisfied level)
  uint32_t flags;    // kFs*
};
enum : uint32_t { kFsSat = 1, kFsMatched = 2, kFsFoundFb = 4, kFsHaveMin = 8, kFsDone = 16 };
struct SampWalkDev;   // devcfg.hpp
struct TraceKernelArgs {
  uint64_t n_spans;
  uint32_t n_windows;         // ceil(n_spans / 64), >= 1
  uint32_t mode;              // kTrace*
  uint32_t n_resources;
  uint32_t epoch;             // hash table generation (>= 1)
  // rule-chunked passes (both null: one pass, the whole rule list): the
  // state before this chunk's rules (null in the first pass) and after them
  // (null in the last pass, which decides), indexed by the trace's first span
  const FoldState* fold_in;
  FoldState* fold_out;
  const uint64_t* tid;
  const uint64_t* start;
  const uint64_t* end;
  const uint8_t* status;
  const uint32_t* resource;
  const ose_strref* route;
  const uint8_t* arena;
  const uint32_t* res_svc;
  const uint32_t* res_svc_str;
  const uint8_t* cfg;         // SampCfgDev blob
  uint64_t seed;
  uint8_t* keep;              // [n_spans]
  TraceRec* rec;              // [max(n,1)] or null (no per-trace outputs)
  uint64_t* win_heads;        // [n_windows] head bitmap of each window
  // slow path
  TraceSlot* table;            // exact table (slow path)
  uint64_t table_mask;
  uint32_t* dup;              // set by the fast path when a trace_id spans several runs
  // bucketed duplicate detection (kTraceRuns): a run head appends its 64-bit fingerprint to bucket fp >> (64 -
  // dup_bkt_bits); trace_dup_check_kernel looks for a repeat per bucket in LDS
  uint32_t* dup_bkt_count;    // [1 << dup_bkt_bits], zeroed before the launch
  uint64_t* dup_bkt;          // [(1 << dup_bkt_bits) * kDupBucketCap]
  uint32_t dup_bkt_bits;
  const uint32_t* perm;       // kTracePerm: position -> span
  const uint32_t* key;        // kTracePerm: span -> canonical trace (first run-head position)
  uint32_t* error;            // bit0 spin timeout, bit2 trace table full
  uint32_t* batch_keep;       // kTraceBatch: the call's decision (read by the SIZE stage)
  const uint64_t* route_match;// optional precomputed endpoint bits (ose_columns.route_match)
  const uint64_t* attr_match; // span_attribute bits (null when no such rule)
  uint64_t attr_stride;       // attr_match: word w of span i at [w * attr_stride + i]
  uint32_t attr_words;
  const uint64_t* svc_match;  // owner-side records: OR of service_name + span_attribute rule bits (replaces both)
  uint32_t ablate;            // diagnostics only (OSE_TRACE_ABLATE, tools/ablate_trace.py): skip parts
  // kTraceRuns: runs still open kLongSteps steps past their owner's windows
  // are listed here (head positions) and decided by trace_long_kernel
  uint32_t* n_long;           // [0] runs listed, [1] pieces, [3] piece partials (trace_long_plan_kernel)
  uint32_t* long_runs;        // [n_spans / 64 + 1]
  // trace_long_plan_kernel cuts each listed run into pieces of at most
  // kLongPiece spans (one workgroup each): per run {end, pieces, first
  // partial, pieces done}, per piece {run, index}, per piece of a run of
  // several a partial (kLongPartBytes)
  uint4* long_meta;           // [n_spans / 64 + 1]
  uint2* long_pieces;         // [long_piece_cap(n_spans)]
  uint8_t* long_part;         // [long_part_cap(n_spans)][kLongPartBytes]
  uint32_t long_steps;        // hand-off distance in 64-span steps (kLongSteps)
  uint32_t win_per_wave;      // 64-span windows whose run heads one wave owns (kWinPerWave)
  uint32_t narrow;            // the table's flag bits fit one word (trace_eval_kernel kNarrow)
  // every rule chunk in one pass (trace_multi_kernel): n_multi (2..kMaxMulti)
  // chunk tables, copied into cfg_lds_bytes of dynamic LDS (0: one table, a.cfg)
  const uint8_t* const* cfgs;
  uint32_t n_multi;
  uint32_t cfg_lds_bytes;     // the tables, then the latency-service ids (lat_gslot)
  const uint32_t* lat_gslot;  // [n_services] index among the latency services, [64] their service ids
  const SampWalkDev* walks;   // [n_multi] each chunk's rules by what matches them
  // run-list path (repeated trace ids, before the sort-based fallback):
  // trace_runs_kernel lists each trace's runs in its exact-table slot,
  // trace_fold_kernel folds the runs of every trace with 2..kMaxRuns runs
  uint32_t* run_count;        // [table slots] runs listed per slot
  uint32_t* runs;             // [table slots * kMaxRuns] run-head positions
  uint32_t* overflow;         // set when a trace needs the sort-based path
  unsigned long long* path_count;   // engine counters (ose_engine_path_counts): [0] += 1 per run-list pass
  uint64_t* win_first;        // [n_windows] heads that start a trace (first run only)
  uint32_t* head_slot;        // [n_spans] exact-table slot of each run head
};
constexpr uint32_t kMaxRuns = 8;          // runs per trace the run-list path folds
constexpr uint32_t kMaxFoldSpans = 4096;  // spans per trace one lane folds
constexpr uint32_t kMaxFoldSlots = 8;     // latency services per trace one lane folds
#ifndef OSE_WPW_BESIDE
#define OSE_WPW_BESIDE 64
#endif
constexpr uint32_t kWinPerWaveBeside = OSE_WPW_BESIDE;   // beside the forked URL planning (sampling_host.cpp)
constexpr uint32_t kWinPerWave = 16;   // tools/gpu_wpw.sh: C5 0.97 -> 0.83 ms, C3 2.03 -> 1.99 ms, C4 unchanged
#ifndef OSE_LONG_PIECE
#define OSE_LONG_PIECE 2048
#endif
constexpr uint32_t kLongPiece = OSE_LONG_PIECE;   // spans of a long run one wave folds
constexpr uint32_t kLongPartBytes = 1344;    // a piece's partial: m[64], e[64], f[64], ep, svc, kmask, err
inline uint64_t long_piece_cap(uint64_t n) { return n / 64 + 1 + n / kLongPiece + 1; }
inline uint64_t long_part_cap(uint64_t n) { return 2 * (n / kLongPiece) + 2; }   // pieces of runs of > kLongPiece spans
constexpr uint32_t kLongSteps = 4;   // tools/gpu_long_iter.sh: C5 16 -> 4 steps 2.75 -> 2.13 ms, C3 unchanged
void launch_trace_eval(const TraceKernelArgs& a, hipStream_t st);
// rule chunks one trace_multi_kernel pass evaluates, and their LDS budget
constexpr uint32_t kMaxMulti = 3;
constexpr uint32_t kMultiCfgLds = 24576;
constexpr uint32_t kDupBucketCap = 1024;   // fingerprints per bucket (more: the exact path decides)
void launch_trace_dup_check(const TraceKernelArgs& a, hipStream_t st);
void launch_trace_long(const TraceKernelArgs& a, hipStream_t st, uint32_t known_runs = 0);
// trace_slow_kernel.hip: the run-list path and the sort path
void launch_trace_insert_exact(const TraceKernelArgs& a, hipStream_t st);   // slow path, gated on *dup
void launch_trace_runs(const TraceKernelArgs& a, hipStream_t st);           // run-list path (gated on *dup)
void launch_trace_fold(const TraceKernelArgs& a, hipStream_t st);
void launch_trace_first_select(const TraceKernelArgs& a, hipStream_t st);   // win_first -> win_heads unless *overflow

// Sort path (trace_slow_kernel.hip; runs only when *gate != 0: every launch checks the flag first).
struct TraceSortArgs {
  uint64_t n_spans;
  uint32_t n_tiles;           // ceil(n / kSortTile)
  uint32_t shift;             // digit shift of this pass
  const uint32_t* gate;       // == TraceKernelArgs::dup
  const uint64_t* tid;
  const TraceSlot* table;
  uint64_t table_mask;
  uint32_t epoch;
  const uint32_t* keys_in;    // null on the first pass: keys_in = key, vals = identity
  const uint32_t* vals_in;
  uint32_t* keys_out;
  uint32_t* vals_out;
  uint32_t* hist;             // [256 * n_tiles] digit-major
  uint32_t* key;              // canonical key per span (trace_key kernel output)
  uint32_t* error;
  unsigned long long* path_count;   // [1] += 1 per call the sort path decided (gate open)
  // sort_hist_kernel zeroes the following scan's tile counter and look-back
  // status (only when the gate is open: no memset launches per closed call)
  uint32_t* scan_counter;
  uint64_t* scan_status;
  uint32_t scan_status_n;
};
constexpr uint32_t kSortTile = 4096;
void launch_trace_key(const TraceSortArgs& a, hipStream_t st);
void launch_sort_hist(const TraceSortArgs& a, hipStream_t st);
void launch_sort_scatter(const TraceSortArgs& a, hipStream_t st);

// Exclusive scan of u32 counts (or popcounts of u64 bitmaps) with the
// decoupled look-back; *total receives the sum.  gate may be null.
struct ScanArgs {
  uint64_t n;
  uint32_t n_tiles;           // ceil(n / kScanTileItems)
  uint32_t popcount;          // 1: input is u64 bitmaps
  const uint32_t* gate;
  const void* in;
  uint32_t* out;
  uint32_t* total;            // may be null
  uint32_t* counter;          // zeroed before launch
  uint64_t* status;           // [n_tiles], zeroed before launch
  uint32_t* error;
};
constexpr uint32_t kScanTileItems = 1024;
void launch_scan_u32(const ScanArgs& a, hipStream_t st);

// Dense per-trace outputs from the records (first-appearance order; trace_slow_kernel.hip).
struct TraceCompactArgs {
  uint32_t n_windows;
  const uint64_t* win_heads;
  const uint32_t* win_base;
  const TraceRec* rec;
  uint32_t* trace_first_span;
  uint8_t* trace_keep;
  uint8_t* trace_level;
  double* trace_ratio;
};
void launch_trace_compact(const TraceCompactArgs& a, hipStream_t st);

// Trace-id exchange (ose_shard_*; shard_kernel.hip).
struct ShardArgs {
  uint64_t n_spans;
  uint32_t n_tiles;           // wave chunks: ceil(n / kXChunk)
  uint32_t n_ranks;           // <= 64
  const uint64_t* tid;
  const uint64_t* start;
  const uint64_t* end;
  const uint8_t* status;
  const uint32_t* resource;
  const ose_strref* route;
  const uint8_t* arena;
  const uint64_t* route_match;
  uint64_t rm_stride;         // route_match: plane k (rule chunk k) at k * rm_stride (0: one plane)
  const uint64_t* attr_match;
  uint64_t attr_stride;       // attr_match: word w of span i at [w * attr_stride + i]
  uint32_t attr_words;
  const uint32_t* res_svc;
  const uint32_t* res_svc_str;
  const uint8_t* const* cfgs;  // [n_chunks] SampCfgDev blobs (device array of the rule chunks' tables)
  uint32_t n_chunks;
  const uint32_t* lat_svc;    // bit s: service s has an http_latency rule in some chunk
  uint32_t n_global_svc;      // services the engine interned (res_svc / res_svc_str / lat_svc index them)
  const uint32_t* const* svc_maps;   // [n_chunks] global -> chunk-local service id (0xFFFFFFFF: not in the
                                     // chunk), or null when every chunk indexes global ids (dense tables)
  uint32_t cfg_lds_bytes;     // the chunk tables copied into LDS by shard_scatter_kernel (sum of their 16-aligned
                              // sizes), 0: read from HBM
  uint32_t* hist;             // [n_ranks * n_tiles] counts, then offsets (second buffer)
  uint32_t* hoff;
  uint64_t* counts;           // [n_ranks] records per owner (shard_counts_kernel)
  uint8_t* send;              // [records * x_rec_bytes(n_chunks)], records <= n
  uint32_t* pack_pos;         // [n] slot of each span's record
};
// Partial record (shard_kernel.hip "trace-id exchange"): u64 words hi, lo,
// min start, max end, {latency service 24 | flags 8}, then per rule chunk
// the endpoint bits and the rule bits of that chunk's tables.
constexpr uint32_t kXSteps = 16;                        // 64-span steps of one packing wave's chunk
constexpr uint32_t kXChunk = kXSteps * 64;              // spans per packing wave
constexpr uint32_t kXFixedWords = 5;
constexpr uint32_t kXRecBytes = 8 * (kXFixedWords + 2);   // a one-chunk config (OSE_XREC_BYTES)
constexpr uint32_t x_rec_words(uint32_t n_chunks) { return kXFixedWords + 2 * n_chunks; }
constexpr uint32_t x_rec_bytes(uint32_t n_chunks) { return 8 * x_rec_words(n_chunks); }
void launch_shard_hist(const ShardArgs& a, hipStream_t st);
void launch_shard_counts(const ShardArgs& a, hipStream_t st);
void launch_shard_scatter(const ShardArgs& a, hipStream_t st);
struct UnpackArgs {
  const uint8_t* recv;
  uint64_t n;
  uint32_t n_chunks;          // route_match / svc_match: n_chunks planes of n words
  uint64_t* tid;
  uint64_t* start;
  uint64_t* end;
  uint8_t* status;
  uint32_t* resource;
  uint32_t* res_svc;
  uint32_t* res_svc_str;
  uint64_t* route_match;
  uint64_t* svc_match;
};
void launch_shard_unpack(const UnpackArgs& a, hipStream_t st);
// Owner-side decisions straight from the received records (ose_shard_decide;
// shard_kernel.hip "owner side"): records bucketed by trace-id hash, one
// workgroup per bucket groups, orders and folds its traces in LDS.
constexpr uint32_t kOwnerCap = 256;   // records one bucket holds (a fuller bucket: the general path)
constexpr uint32_t kOwnerAvg = 80;    // records per bucket the host sizes the bucket count for
// a bucket slot, 64 bytes written and read as four uint4 (owner_bucket_kernel / owner_fold_kernel):
// {hi, lo} | {min start, max end} | {w4 : 32, record index : 32, chunk 0's endpoint word} | {chunk 0's rule word, 0}
constexpr uint32_t kOwnerSlotWords = 8;
struct OwnerArgs {
  const uint8_t* recv;        // n records of x_rec_words(n_chunks) words, in (source rank, source order)
  uint64_t n;
  uint32_t words;
  uint32_t n_buckets;
  uint32_t* bkt_count;        // [n_buckets], zeroed before the bucket pass
  uint64_t* bkt_rec;          // [n_buckets * kOwnerCap * kOwnerSlotWords] the records' slots
  const uint8_t* const* cfgs; // [n_chunks] SampCfgDev blobs
  uint32_t n_chunks;
  const uint32_t* const* svc_maps;   // as ShardArgs::svc_maps (records carry global service ids)
  uint32_t n_global_svc;
  uint32_t cfg_lds_bytes;     // dynamic LDS: the largest chunk table without its route bytes (16-aligned)
  uint64_t seed;
  uint8_t* keep;              // [n] per record
  uint32_t* overflow;         // set: a bucket past kOwnerCap records
  uint64_t* clocks;           // OSE_DIAG builds: per-phase clocks of owner_fold_kernel (OSE_OWNER_CLOCKS), else null
};
void launch_owner_bucket(const OwnerArgs& a, hipStream_t st);
void launch_owner_fold(const OwnerArgs& a, hipStream_t st);
void launch_scatter_keep(const uint8_t* back, const uint32_t* pos, uint64_t n, uint8_t* keep, hipStream_t st);
// trace_kernel.hip, per rule chunk:
// out[r] = map[in[r]] (0xFFFFFFFF for ids >= n_global), for res_svc and res_svc_str
void launch_svc_translate(const uint32_t* map, uint32_t n_global, const uint32_t* in1, const uint32_t* in2, uint32_t* out1,
                          uint32_t* out2, uint64_t n, hipStream_t st);
// endpoint bits of every span under one rule chunk's tables in HBM (a chunk
// whose route bytes spill past the LDS copy): out[j] for span j
void launch_endpoint_plane(const uint8_t* cfg, const uint32_t* resource, const uint32_t* res_svc, const ose_strref* route,
                           const uint8_t* arena, uint64_t n, uint64_t* out, hipStream_t st);
// the in-process transport's pieces of one phase, moved by one launch (shard_kernel.hip)
struct PeerCopies {
  const uint8_t* src[64];
  uint8_t* dst[64];
  uint64_t len[64];
  uint32_t n;
};
void launch_peer_copies(const PeerCopies& c, uint64_t max_len, hipStream_t st);
// dst[k] += src[k] (the in-process transport's counter all-reduce)
void launch_add_i64(int64_t* dst, const int64_t* src, uint64_t n, hipStream_t st);
uint32_t shard_owner_host(uint64_t hi, uint64_t lo, uint32_t n_ranks);

// Workspace words shared between stages of one call (uint32 index into the
// first 256 bytes of the workspace; URL uses words 0-3, SAMPLE 0-15).
constexpr uint32_t kBatchKeepWord = 16;   // OSE_GROUP_BATCH decision of the SAMPLE stage

// odigostrafficmetrics (size_kernel.hip): three passes, spans -> scopes ->
// resources, each a wave-segmented reduction (the columns are in pdata
// order, so scope and resource indices are non-decreasing).
void launch_size_spans(const SizeKernelArgs& a, hipStream_t st);
// scopes and resources in one pass (size_tail_kernel: every resource whose
// scopes lie in one 64-scope window is finished there), then the resources
// whose scopes span windows (size_fix_kernel)
void launch_size_tail(const SizeKernelArgs& a, hipStream_t st);
void launch_size_fix(const SizeKernelArgs& a, hipStream_t st);

// odigossqldboperationprocessor (sqlop_kernel.hip): one lane per span,
// sql_op[i] = OSE_SQLOP_* of db_query[i] where db_flags[i] is HAS_QUERY
// without HAS_OPNAME and the span's resource passes res_sql_ok, else 0.
struct SqlOpArgs {
  uint64_t n_spans;
  const uint8_t* arena;
  const uint8_t* db_flags;
  const ose_strref* db_query;
  const uint32_t* resource;
  const uint8_t* res_sql_ok;   // may be null (no exclude list)
  uint8_t* sql_op;
};
void launch_sqlop(const SqlOpArgs& a, hipStream_t st);
// The spans pass of the size stage after SQLOP / APPLY_SQLOP: size_span_kernel
// plus the KeyValue and the longer name of the spans with sql_op != 0.
// sz.name_len is read whether or not sz.templated is set.
struct SqlSizeArgs {
  SizeKernelArgs sz;
  const uint8_t* sql_op;
};
void launch_sqlop_size_spans(const SqlSizeArgs& a, hipStream_t st);

// odigosconditionalattributes (condattr_kernel.hip): the scope prepass (one
// lane per scope, fills scratch) and the span kernel (one lane per span,
// grid-stride), both running the steps of condattr_device.hpp over the
// compiled config blob.
struct CondAttrArgs {
  const uint8_t* blob;
  ose_condattr_columns c;
  ose_condattr_outputs o;
};
void launch_condattr_scopes(const CondAttrArgs& a, hipStream_t st);
void launch_condattr_spans(const CondAttrArgs& a, hipStream_t st);

// span_attribute conditions (attr_kernel.hip): out[i] = host_bits[i] &
// host_mask | the bits of the GPU-evaluated rules the span meets.
struct AttrArgs {
  uint64_t n_spans;
  const uint8_t* type;         // [n_keys * n_spans] OSE_ATTR_*
  const uint64_t* val;         // [n_keys * n_spans]
  const uint8_t* arena;
  const uint32_t* resource;
  const uint32_t* res_svc;
  uint32_t words;              // attr_match words per span (word-major planes of n_spans)
  const uint64_t* host_bits;   // may be null
  const uint64_t* host_mask;   // [words] the shim-evaluated rules
  const uint8_t* cfg;          // AttrCfgDev blob
  uint64_t* out;
};
void launch_attr_eval(const AttrArgs& a, hipStream_t st);

// OTLP protobuf ingest (otlp_kernel.hip).  Attribute keys the decoder
// looks for, with the roles a key plays (one entry per distinct key).
enum : uint32_t {
  kRoleMethodNew = 1u << 0,   // http.request.method
  kRoleMethodOld = 1u << 1,   // http.method
  kRoleRoute = 1u << 2,       // http.route (sampling route; SERVER target)
  kRoleUrlTmpl = 1u << 3,     // url.template (CLIENT target)
  kRoleUrlPath = 1u << 4,     // url.path
  kRoleTarget = 1u << 5,      // http.target
  kRoleFull = 1u << 6,        // url.full / http.url: net/url.Parse on the host (otlp_url_full: otlp_url_full_kernel.hip)
  kRoleHost = 1u << 7,        // a json span_attribute rule's key: host pass
};
constexpr uint64_t kRoleAttr0 = 1ull << 8;   // << k: GPU attribute key column k (k < kOtlpMaxAttrKeys)
constexpr uint32_t kOtlpMaxAttrKeys = 56;
struct OtlpKeyDev {
  uint32_t len, off;
  uint64_t roles;
};
struct OtlpArgs {
  const uint8_t* pb;            // message bytes = the arena (16-byte aligned, 16 bytes of slack)
  uint64_t n_spans;
  const uint64_t* span_ref;     // payload offset | length << 32
  const OtlpKeyDev* keys;
  const uint8_t* key_bytes;
  uint32_t n_keys;
  uint32_t n_attr_keys;
  uint64_t key_lens;            // bit min(l, 63): some key has length l (a filter: the per-key compare is exact)
  uint64_t* tid;
  uint64_t* start;
  uint64_t* end;
  uint8_t* status;
  uint8_t* kind;
  uint8_t* url_flags;
  ose_strref* path;
  ose_strref* route;
  uint32_t* span_size;
  uint32_t* name_len;
  uint64_t* attr_match;         // may be null; attr_words word-major planes of n_spans
  uint32_t attr_words;
  uint8_t* attr_type;
  uint64_t* attr_val;
  uint8_t* host_flag;           // [n_spans] 1 = the host pass writes this span
  uint32_t* host_count;         // zeroed before launch
  uint32_t* host_list;
  uint32_t host_cap;
  uint32_t url_full;            // engine option otlp_url_full: a url.full / http.url source alone lists no span
};
// ScopeSpans walked on the GPU (the host walks TracesData and ResourceSpans
// only): pass 1 counts each scope's spans and reads its InstrumentationScope
// and schema_url; pass 2 (after a scan of the counts) writes the span refs.
constexpr uint64_t kOtlpScopeMulti = ~0ull;
struct OtlpScopeArgs {
  const uint8_t* pb;
  uint64_t n_scopes;
  const uint64_t* scope_ref;    // ScopeSpans payload off | len << 32
  const uint8_t* on_host;       // 1: the host walked this scope (counts / sizes / layout preset)
  const uint32_t* scope_res;
  uint32_t* count;              // spans per scope
  uint32_t* scope_size;         // pdata's fixed ScopeSpans size (scope + schema_url)
  uint64_t* hdr;                // the InstrumentationScope message ref, 0 none, kOtlpScopeMulti several
  uint64_t* schema;             // schema_url ref (last occurrence; length 0: none)
  uint32_t* flags;              // 1: size left to the host (merged / unusual scope message), 2: malformed
  const uint32_t* span0;        // pass 2: exclusive scan of count
  uint64_t* span_ref;
  uint32_t* span_res;
  uint32_t* span_scope;
  // pass 2 for the host-walked scopes: their refs, listed in scope order
  const uint64_t* host_refs;
  const uint64_t* host_at;      // [n_scopes] offset into host_refs (host-walked scopes)
};
// ResourceSpans on the GPU (the host walks only the TracesData chain of
// ResourceSpans records): each record's fields, its Resource's columns from
// the engine's device table of resources seen before (keyed by the Resource
// message bytes: FNV-1a 64), its ScopeSpans listed for the scope passes.
struct ResSlotDev {          // 48 B; ready != 0: filled
  uint64_t h;
  uint32_t koff, klen;       // key bytes in the table's key arena
  uint32_t svc, svc_str, set, rpart;
  uint64_t attr_res;
  uint32_t ok, ready;        // ok: bit 0 res_url_ok, bit 1 res_sql_ok
};
constexpr uint32_t kResSlots = 1u << 17;
constexpr uint32_t kResKeyBytes = 16u << 20;
// FNV-1a over the bytes (the host fills the table with the same function)
inline __host__ __device__ uint64_t res_key_hash_step(uint64_t h, uint32_t b) { return (h ^ b) * 0x100000001B3ull; }
constexpr uint64_t kResHashSeed = 0xCBF29CE484222325ull;
struct OtlpResArgs {
  const uint8_t* pb;
  uint64_t n_res;
  const uint64_t* res_ref;     // ResourceSpans payload off | len << 32
  uint32_t* flags;             // 1: resource columns from the host, 2: malformed, 4: scopes are field 1000
  uint32_t* nscope;            // ScopeSpans per resource (field 2, or field 1000 when there is no field 2)
  uint32_t* schema_len;        // ResourceSpans.schema_url length (last occurrence)
  uint32_t* any_bad;           // [1] OR of flags & 2
  const uint32_t* scope0;      // pass 2: exclusive scan of nscope
  uint64_t* scope_ref;
  uint32_t* scope_res;
  // the Resource's columns
  const ResSlotDev* table;
  const uint8_t* keys;
  uint32_t* res_svc;
  uint32_t* res_svc_str;
  uint32_t* res_set;           // the resource cache's attribute-set id (batch ids after compaction)
  uint32_t* res_size;
  uint8_t* res_ok;
  uint8_t* res_sql_ok;         // may be null (engine option otlp_sqlop off)
  uint64_t* attr_res;
  uint32_t* miss_count;        // [1]
  uint32_t* miss_list;         // [n_res]
};
// The TracesData chain on the GPU: the message split into segments of
// kChainSeg bytes; lane t speculates a record start in its segment (as the
// host walk's find_start does) and walks the top-level fields from it until
// the first field boundary at or past the next segment.  The host links the
// segments (a speculated start inside a record converges to the true chain at
// that record's end, one of the field starts listed) and otlp_chain_list
// writes the records of each linked segment from its first true field on.
constexpr uint32_t kChainSeg = 64u << 10;
constexpr uint32_t kChainList = 16;   // field starts listed per segment
constexpr uint64_t kChainNone = ~0ull;
struct OtlpChainArgs {
  const uint8_t* pb;
  uint64_t n;
  uint32_t n_seg;
  uint64_t* start;      // [n_seg] speculated start (kChainNone: none in the segment)
  uint64_t* end;        // [n_seg] where the walk stopped (first boundary >= next segment)
  uint32_t* nrec;       // [n_seg] records (field 1) walked
  uint32_t* bad;        // [n_seg] the walk met a malformed field (end = where)
  uint64_t* list;       // [n_seg * kChainList] field starts | (field 1) << 63
  // pass 2 (linked segments): walk from first[t] (kChainNone: skip), records to res_ref from base[t]
  const uint64_t* first;
  const uint32_t* base;
  uint64_t* res_ref;
};
void launch_otlp_chain_seg(const OtlpChainArgs& a, hipStream_t st);
void launch_otlp_chain_list(const OtlpChainArgs& a, hipStream_t st);
void launch_otlp_res_fields(const OtlpResArgs& a, hipStream_t st);
void launch_otlp_res_scopes(const OtlpResArgs& a, hipStream_t st);
// the host's columns of the missed resources: fix k = {row, svc, svc_str, set, rpart, ok, attr_res}
// (ok as in ResSlotDev: bit 0 res_url_ok, bit 1 res_sql_ok)
struct OtlpResFix {
  uint32_t row, svc, svc_str, set, rpart, ok;
  uint64_t attr_res;
};
void launch_otlp_res_fix(const OtlpResArgs& a, const OtlpResFix* fix, uint32_t n, hipStream_t st);
// attribute-set ids of the cache -> the batch's, in order of first appearance
// (as the host walk numbers them): each set's first resource (first[], set
// to ~0 before), the resources that are first of their set (is_first), and
// after an exclusive scan of those flags (pos) the ids and the batch's list
void launch_otlp_set_first(const uint32_t* res_set, uint64_t n_res, uint32_t* first, uint32_t* is_first,
                           hipStream_t st);
void launch_otlp_set_apply(uint32_t* res_set, uint64_t n_res, const uint32_t* first, const uint32_t* is_first,
                           const uint32_t* pos, uint32_t* list, hipStream_t st);
void launch_otlp_scope_count(const OtlpScopeArgs& a, hipStream_t st);
void launch_otlp_scope_spans(const OtlpScopeArgs& a, hipStream_t st);

// OTLP re-encode on the GPU (encode_kernel.hip): the
// sizing and writing passes of otlp_encode.cpp over the message bytes and
// the decisions, both already in HBM.  Resources are routed on the device
// (odigosrouterconnector's key from the Resource's attributes, looked up in
// an FNV-1a table of the router's keys).  What the device path does not
// write exactly as the host encoder would — a span, scope or resource whose
// encoding is not already pdata's, a method needing AsString, fields out of
// order, a merged Resource — sets a flag, and the call goes to the host
// encoder instead.
constexpr uint64_t kEncDropped = ~0ull;
constexpr uint64_t kEncNoHdr = ~0ull;            // res_hdr / scope header: absent ("0A 00")
constexpr uint32_t kEncTiles = 1024;             // resources per scan tile
enum : uint32_t {
  kEncFbSpan = 1,       // a rewritten span pdata would re-marshal, or an AsString method
  kEncFbScope = 2,      // a scope header not in pdata's encoding / merged
  kEncFbRes = 4,        // a resource header not in pdata's encoding / merged / malformed
  kEncFbTmpl = 8,       // a template reference beyond the arena (the host reports it)
  kEncFbRoute = 16,     // a routing attribute the device does not read exactly
  kEncFbWrite = 32,     // the writing pass disagreed with the sizing pass (a bug: the call fails)
  kEncFbCa = 64,        // odigosconditionalattributes: more targets than kEncCaTargets, or a put the host
                        // reports (a src beyond OSE_CA_CONFIG, a ref beyond its buffer)
};
struct EncEdit {        // one rewritten span (otlp_encode.cpp Edit)
  uint32_t name_a, name_b, attr_a, attr_b;
  uint32_t meth_off, meth_len;   // the method string in the message
  uint32_t tmpl_off, tmpl_len;   // the template in the template arena
  uint32_t out_len;              // edited span bytes
  uint32_t flags;                // url_out | client << 8 | sql_op << 16
};
// ... and what a sql_op adds to the plan (a call with OSE_STAGE_SQLOP /
// OSE_STAGE_APPLY_SQLOP; kernels of their own, so a call without runs the
// code it ran before): the db.operation.name KeyValue replaced (sql_a <
// sql_b) or inserted (sql_a == sql_b), and the span's own name (field 5's
// payload, in the message), which the new name starts with unless the URL
// stage renamed the span
struct EncSqlEdit {
  uint32_t sql_a, sql_b;
  uint32_t own_off, own_len;
};
struct EncRouteSlot {   // router key "ns/kind/name" -> pipelines; klen == ~0: empty
  uint64_t h;
  uint32_t koff, klen;
  uint64_t mask;
};
struct EncArgs {
  const uint8_t* pb;
  uint64_t n_spans, n_scopes, n_res;
  const uint64_t* span_ref;
  const uint32_t* span_size;
  const uint8_t* keep;           // NULL: every span kept
  const uint8_t* url_out;        // NULL: no template stage
  const ose_strref* tmpl;
  const uint8_t* tmpl_arena;
  const uint64_t* tmpl_used;
  const uint8_t* sql_op;         // NULL: no odigossqldboperationprocessor stage
  EncSqlEdit* sql_edit;          // [n_spans] with sql_op
  const uint32_t* scope_span0;
  const uint64_t* scope_hdr;     // InstrumentationScope ref (0: none, kOtlpScopeMulti: merged)
  const uint64_t* scope_schema;
  const uint32_t* scope_size;    // the decoder's pdata size of the scope's fixed part
  const uint64_t* res_ref;
  const uint32_t* res_scope0;
  const uint32_t* res_size;      // the decoder's pdata size of the resource's fixed part
  uint32_t n_out;                // router pipelines + 1 (default), or 1
  uint32_t route_bits;           // log2 of the route table's slots (0: no router)
  const EncRouteSlot* routes;
  const uint8_t* route_keys;
  // sizing pass
  uint32_t* span_out;            // framed bytes of span i in its scope (0: dropped)
  EncEdit* edit;
  uint64_t* scope_body;          // kEncDropped: removed
  uint64_t* res_body;
  uint64_t* res_rec;             // framed record bytes (0: dropped)
  uint64_t* res_mask;            // outputs the resource goes to
  uint64_t* res_hdr;             // Resource payload ref, kEncNoHdr: absent
  uint64_t* res_schema;          // ResourceSpans.schema_url ref (length 0: none)
  uint32_t* flags;               // [1] OR of kEncFb*
  // scans: offsets per output, then the writing pass
  uint64_t* tile_sum;            // [n_out][tiles] bytes, then [n_out][tiles] counts
  uint64_t* off;                 // [n_out][n_res]
  uint64_t* out_total;           // [n_out] bytes, then [n_out] resource counts
  const uint64_t* out_base;      // [n_out]
  uint8_t* out;
};
void launch_enc_spans(const EncArgs& a, hipStream_t st);
void launch_enc_scopes(const EncArgs& a, hipStream_t st);
void launch_enc_resources(const EncArgs& a, hipStream_t st);
void launch_enc_scan(const EncArgs& a, hipStream_t st);
void launch_enc_write(const EncArgs& a, hipStream_t st);
// ... and the instances of ose_otlp_encode_condattr (enc_span_ca_kernel /
// enc_write_ca_kernel): odigosconditionalattributes' puts, src / val as
// ose_condattr_outputs (device), the names in the engine's compiled config.
// The GPU path takes configs of up to kEncCaTargets targets: a span's puts
// are a bit mask held in a register through the sizing and the writing walk
// (below 32: ca_match answers 32 for "none"; the shipped category-attributes
// profile has 3 targets, the tests' adversarial config 17); a config with more
// goes to the host encoder (kEncFbCa), which has no such bound.
constexpr uint32_t kEncCaTargets = 24;
struct EncCaArgs : EncArgs {
  const uint8_t* ca_blob;        // condattr_device.hpp's blob
  const uint8_t* ca_src;         // [ca_targets * n_spans]
  const ose_strref* ca_val;
  uint32_t ca_targets;
  uint32_t ca_string_bytes;      // the blob's string table
  uint64_t ca_arena_bytes;       // the batch arena (pb is its base)
  uint32_t* ca_len;              // [n_spans] the new length of a span with puts
};
void launch_enc_spans_ca(const EncCaArgs& a, hipStream_t st);
void launch_enc_write_ca(const EncCaArgs& a, hipStream_t st);

struct OtlpFix {
  uint64_t idx;
  uint64_t hi, lo, start, end;
  ose_strref path, route;
  uint32_t span_size, name_len;
  uint8_t status, kind, url_flags, _pad[5];
};
struct OtlpFixArgs {
  uint32_t n;
  uint32_t n_attr_keys;
  uint64_t n_spans;
  const OtlpFix* fix;
  uint32_t attr_words;          // attr_match words per span (fix_attr: [n * attr_words])
  const uint64_t* fix_attr;
  const uint8_t* fix_type;      // [n * n_attr_keys]
  const uint64_t* fix_val;
  uint64_t* tid;
  uint64_t* start;
  uint64_t* end;
  uint8_t* status;
  uint8_t* kind;
  uint8_t* url_flags;
  ose_strref* path;
  ose_strref* route;
  uint32_t* span_size;
  uint32_t* name_len;
  uint64_t* attr_match;
  uint8_t* attr_type;
  uint64_t* attr_val;
};
uint32_t launch_otlp_spans(const OtlpArgs& a, hipStream_t st);   // the kernel launched: 0 none, 1 LDS-staged, 2 HBM
void launch_otlp_fix(const OtlpFixArgs& a, hipStream_t st);

// odigossqldboperationprocessor's span columns from the message
// (otlp_sqlop_kernel.hip; engine option otlp_sqlop).  A pass of its own after
// the span kernel, one lane per span: db_flags, and db_query as a ref into
// the message bytes when db.query.text is a string_value.  Any other value
// needs AsString: the span joins the host pass's list (unless the span kernel
// listed it already), and the host pass writes both columns of every listed
// span (OtlpSqlFix, after OtlpFix).
struct OtlpSqlArgs {
  const uint8_t* pb;            // as OtlpArgs::pb
  uint64_t n_spans;
  const uint64_t* span_ref;
  uint8_t* db_flags;
  ose_strref* db_query;
  uint8_t* host_flag;           // the span kernel's; 1: skipped here
  uint32_t* host_count;
  uint32_t* host_list;
  uint32_t host_cap;
};
void launch_otlp_sqlop(const OtlpSqlArgs& a, hipStream_t st);
struct OtlpSqlFix {
  uint32_t idx, flags;
  ose_strref query;
};
void launch_otlp_sqlop_fix(const OtlpSqlFix* fix, uint32_t n, uint8_t* db_flags, ose_strref* db_query, hipStream_t st);

// The Path of net/url.Parse(url.full | http.url) from the message
// (otlp_url_full_kernel.hip, url_full.hpp; engine option otlp_url_full).  A
// pass of its own after the span kernel, one lane per span it finished with
// OSE_URL_HAS_METHOD and OSE_URL_PATH_NONE: the first url.full KeyValue, else
// the first http.url.  A value that is not a string_value needs AsString: the
// span joins the host pass's list.  A Path without escapes is a ref into the
// message bytes (OSE_URL_PATH_RAW); one with escapes parks its raw sub-range
// in path[i] and its decoded length in dec_len[i].  After a scan of dec_len
// (dec_off) and room in the arena, launch_otlp_url_full_unescape writes the
// decoded bytes at arena + dec_base + dec_off[i] and points path[i] there.
struct OtlpUrlFullArgs {
  const uint8_t* pb;            // as OtlpArgs::pb
  uint64_t n_spans;
  const uint64_t* span_ref;
  uint8_t* url_flags;
  ose_strref* path;
  uint32_t* dec_len;            // [n_spans] written for every span (0: nothing to unescape)
  const uint32_t* dec_off;      // the unescape pass: exclusive scan of dec_len
  uint32_t* parsed;             // += the spans whose string value was parsed here (zeroed before launch)
  uint8_t* out;                 // the unescape pass: the arena (pb may be the same buffer; the regions are disjoint)
  uint32_t dec_base;
  uint8_t* host_flag;           // the span kernel's; 1: skipped here
  uint32_t* host_count;
  uint32_t* host_list;
  uint32_t host_cap;
};
void launch_otlp_url_full(const OtlpUrlFullArgs& a, hipStream_t st);
void launch_otlp_url_full_unescape(const OtlpUrlFullArgs& a, hipStream_t st);

// odigosconditionalattributes' span columns from the message
// (otlp_condattr_kernel.hip; engine option otlp_condattr).  A pass of its own
// after the span kernel (and otlp_sqlop_kernel), one lane per span: for the
// first attributes KeyValue of each of the engine's condattr keys span_has = 1,
// span_val a ref into the message bytes and, for target keys, span_kv_size.
// span_has is zeroed before the launch; only hits are stored.  The keys are
// found through a table built when the option is set (OtlpCaSlot[mask + 1],
// open addressing on the key bytes' FNV-1a, load <= 1/2; key_lens: bit
// min(len, 63) per key length) over the Key[] and strings of the compiled
// config's blob (condattr_device.hpp).  A matched key whose value is not a
// string_value needs AsString: the span joins the host pass's list (unless
// listed already), and the host pass writes all K entries of every listed span
// (otlp_condattr_fix_kernel).
struct OtlpCaSlot { uint32_t hash, key; };   // key == 0xFFFFFFFF: empty
struct OtlpCondAttrArgs {
  const uint8_t* pb;            // as OtlpArgs::pb
  uint64_t n_spans;
  const uint64_t* span_ref;
  const uint8_t* blob;          // the engine's compiled config on the device
  const OtlpCaSlot* slots;
  uint32_t slot_mask;
  uint64_t key_lens;
  uint8_t* span_has;            // [K * n_spans], key-major
  ose_strref* span_val;
  uint32_t* span_kv_size;
  uint8_t* host_flag;           // the span kernel's; 1: skipped here
  uint32_t* host_count;
  uint32_t* host_list;
  uint32_t host_cap;
};
void launch_otlp_condattr(const OtlpCondAttrArgs& a, hipStream_t st);
// the host pass's entries, [k * cnt + q] for key k of listed span list[q]
struct OtlpCondAttrFixArgs {
  uint32_t cnt, n_keys;
  uint64_t n_spans;
  const uint32_t* list;         // the host list (device)
  const uint8_t* fix_has;
  const ose_strref* fix_val;
  const uint32_t* fix_kv;
  uint8_t* span_has;
  ose_strref* span_val;
  uint32_t* span_kv_size;
};
void launch_otlp_condattr_fix(const OtlpCondAttrFixArgs& a, hipStream_t st);

// ---- groupbytrace store (gbt_kernel.hip) --------------------------------------
struct GbtSlot {              // trace id -> creation number (32 B, generation-tagged)
  uint32_t state;             // epoch << 2 | {0 empty, 1 busy, 2 ready}
  uint32_t first;             // smallest batch position carrying the id (new ids)
  uint64_t hi, lo;
  uint64_t seq;               // creation number of the id's newest trace; kGbtUnset | add
                              // while add number `add` is numbering a new trace for it
};
constexpr uint64_t kGbtUnset = 0xFFFFFFFF00000000ull;
// GbtArgs::error bits
constexpr uint32_t kGbtErrSpin = 1;      // a slot stayed busy past the spin limit
constexpr uint32_t kGbtErrProbe = 4;     // a table probe overran the table
constexpr uint32_t kGbtErrRefused = 8;   // the batch is refused: the arena ring is full
constexpr uint32_t kGbtErrHeader = 16;   // a ResourceSpans / ScopeSpans header not walked
struct GbtPool {              // spans waiting for release (ring of pool_cap)
  uint64_t* tid;              // {hi, lo}
  uint64_t *start, *end, *attr_match, *seq, *origin, *str_off;
  uint8_t *status, *kind, *url_flags;
  uint32_t *span_size, *name_len;
  ose_strref *route, *path;   // relative to the span's string block
  uint8_t* attr_type;         // key-major, [key * pool_cap + p]
  uint64_t* attr_val;
  // odigossqldboperationprocessor (GbtArgs::sql; NULL otherwise): the query
  // is the last string of the block, {0, 0} without OSE_DB_HAS_QUERY
  uint8_t* db_flags;
  ose_strref* db_query;
};
struct GbtScopes {            // the fragment columns of each added scope (ring)
  uint32_t *res_svc, *res_svc_str, *res_attrset, *res_size, *scope_size;
  uint8_t* res_url_ok;
  uint8_t* res_sql_ok;        // GbtArgs::sql
};
struct GbtOut {               // the released batch
  uint64_t* tid;
  uint64_t *start, *end, *attr_match;
  uint8_t *status, *kind, *url_flags;
  uint32_t *span_size, *name_len, *resource, *scope;
  ose_strref *route, *path;
  uint8_t* attr_type;
  uint64_t* attr_val;
  uint32_t *res_svc, *res_svc_str, *res_attrset, *res_size, *scope_size, *scope_resource;
  uint8_t* res_url_ok;
  uint8_t* arena;
  uint8_t* db_flags;          // GbtArgs::sql: the three columns of OSE_STAGE_SQLOP
  ose_strref* db_query;
  uint8_t* res_sql_ok;
};
// OTLP mode (ose_gbt_add_otlp / ose_gbt_release_otlp): a span's block in the
// arena ring is [Span message][strings as in columns mode], and every added
// scope has a header block there too: its ResourceSpans payload without the
// scope_spans fields, then its ScopeSpans payload without the spans fields.
struct GbtOtlp {
  uint32_t on;                  // the launches pick the kernels' OTLP instances
  // add: the batch's layout (device), per-scope header lengths and their scan
  const uint64_t* span_ref;     // [n] Span payload off | len << 32 in cols.arena
  const uint64_t* res_ref;      // [n_resources] ResourceSpans payload
  const uint64_t* scope_ref;    // [n_scopes] ScopeSpans payload
  uint32_t *hres, *hscope;      // [n_scopes] bytes of the two header parts
  uint32_t *hlen, *hoff;        // [n_scopes] their sum, its exclusive scan
  uint64_t* total64;            // [0] bytes of the call's blocks and header blocks (never wraps)
  // the rings
  uint32_t* msg_len;            // pool: the message is the first msg_len bytes of the block
  uint64_t* hdr_off;            // scope ring: the header block's arena position
  uint32_t *hdr_res, *hdr_scope;   // scope ring: bytes of its two parts
  // release: what the GPU encoder reads, per span / per fragment
  uint64_t* out_span_ref;
  uint32_t *out_span0, *out_res_scope0;
  uint64_t *out_hdr, *out_schema, *out_res_ref, *out_scope_ref;
};
struct GbtArgs {
  GbtSlot* table;
  uint64_t table_mask;
  uint32_t epoch;
  uint32_t n_attr_keys;
  uint32_t* error;
  uint64_t* ring_tid;         // [2 * ring_n]: the id of trace seq at seq % ring_n
  uint64_t num_traces;
  uint64_t ring_n;            // num_traces (one worker), else the pool capacity
  // num_workers > 1 (contrib's event machine): trace seq belongs to worker
  // fnv64(id) % n_workers, numbered q within it; tinfo[seq % ring_n] =
  // worker << 40 | q.  It is evicted once its worker has numbered more
  // than q + worker_cap traces (wcnt: the workers' counts the call sees)
  uint32_t n_workers;
  uint64_t worker_cap;
  uint64_t* tinfo;
  const uint64_t* wcnt;
  uint32_t *wadd, *wstart;    // numbering: creators per worker in the batch, their exclusive scan
  uint64_t live_lo, live_hi;  // traces an added span may join (and the rebuild range)
  uint32_t add_gen;           // number of this add (tags the ids it numbers)
  uint32_t attr_words;        // attr_match words per span (word-major: batch, pool and released planes)
  uint64_t arena_room;        // string bytes the arena ring can still take
  const uint32_t* totals;     // [0] new traces, [1] string bytes of the batch (scans)
  // add: the batch
  ose_columns cols;
  uint64_t n, n_scopes;
  uint64_t next_seq;
  uint64_t* slot_of;
  uint32_t *flag, *rank, *strlen, *stroff;
  const uint32_t* attrset_map;
  // the rings
  GbtPool pool;
  uint64_t pool_pos, pool_cap;
  GbtScopes scopes;
  uint64_t scope_pos, scope_cap;
  uint8_t* arena_ring;
  uint64_t arena_pos, arena_cap;
  // release
  uint64_t rel_lo, rel_hi;
  uint32_t *keys, *vals;
  const uint32_t* order;
  GbtOut out;
  // the engine has the odigossqldboperationprocessor section: the store
  // carries db_flags / db_query / res_sql_ok (the launches pick the kernels'
  // SQL instances; without it they are the instances that never read these)
  uint32_t sql;
  // a store fed by ose_gbt_add_otlp (at the end: the fields above keep their
  // offsets, and a columns-mode store never reads these)
  GbtOtlp otlp;
};
void launch_gbt_rebuild(const GbtArgs& a, hipStream_t st);
void launch_gbt_lookup(const GbtArgs& a, hipStream_t st);
void launch_gbt_creator(const GbtArgs& a, hipStream_t st);
void launch_gbt_assign(const GbtArgs& a, hipStream_t st);
void launch_gbt_append(const GbtArgs& a, hipStream_t st);
void launch_gbt_strings(const GbtArgs& a, hipStream_t st);
void launch_gbt_scopes(const GbtArgs& a, hipStream_t st);
void launch_gbt_flag(const GbtArgs& a, hipStream_t st);
void launch_gbt_compact(const GbtArgs& a, hipStream_t st);
void launch_gbt_gather(const GbtArgs& a, hipStream_t st);
void launch_gbt_emit(const GbtArgs& a, hipStream_t st);
// GbtArgs::sql only, one wave per 64 spans moving bytes together: the added
// batch's queries into the arena ring (after launch_gbt_creator's lengths are
// scanned), the released spans' string blocks out of it (beside launch_gbt_emit)
void launch_gbt_query_copy(const GbtArgs& a, hipStream_t st);
void launch_gbt_block_copy(const GbtArgs& a, hipStream_t st);
// OTLP mode: the added scopes' header lengths (before their scan); the call's
// byte total in 64 bits (n = spans of the add, or released spans); the
// messages and header blocks into the ring; the released fragments'
// InstrumentationScope / schema_url refs out of their moved header blocks
void launch_gbt_hdr_len(const GbtArgs& a, hipStream_t st);
void launch_gbt_total(const GbtArgs& a, hipStream_t st);
void launch_gbt_msg_copy(const GbtArgs& a, hipStream_t st);
void launch_gbt_hdr_copy(const GbtArgs& a, hipStream_t st);
void launch_gbt_frag_hdr(const GbtArgs& a, uint64_t n_frag, hipStream_t st);
void launch_gbt_wkey(const GbtArgs& a, hipStream_t st);                 // creators -> (worker, rank) pairs
void launch_gbt_wnum(const GbtArgs& a, uint64_t created, hipStream_t st);   // sorted pairs -> tinfo

}  // namespace ose
