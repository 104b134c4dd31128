// url_host.cpp — odigosurltemplate: the table compiler (build_url_blob), the
// stage's workspace layout and its launch sequence (url_kernel.hip) in two
// halves: run_url queues the front (plan, slow plan, scan, slow emit), which
// reads nothing another stage writes, and run_url_back the copy, which
// run_stages may fuse with odigostrafficmetrics' spans pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/odigos_amd.h"
#include "blob.hpp"
#include "config.hpp"
#include "devcfg.hpp"
#include "engine_internal.hpp"
#include "kernels.hpp"
#include "regex_dfa.hpp"
#include "regex_nfa.hpp"
#include "slab.hpp"

namespace ose {

// odigosurltemplate tables: newUrlTemplateProcessor (processor.go:27-69)
// groups rules by segment count keeping config order; custom ids default
// their name to "id".
// A regexp goes to the DFA compiler first, with its caps; only TooLarge (the
// state or table cap after the subset construction ran into it, seconds per
// such regexp; or more than 255 rune classes, at once) sends it to the NFA
// compiler (regex_nfa.hpp), so a regexp with a DFA keeps its table.
// force_nfa (engine option url_regex_nfa): every regexp as an NFA program.
// nfa_words: the widest program's state words (0: the tables hold no NFA).
int build_url_blob(const UrlTemplateConfig& c, std::vector<uint8_t>& out, uint32_t& max_name, bool force_nfa,
                   uint32_t& nfa_words) {
  Blob bl;
  UrlCfgDev h{};
  bl.put(&h, 1);
  std::string bytes;
  std::vector<NameDev> names;
  auto add_text = [&](const std::string& s) {
    NameDev n{(uint32_t)bytes.size(), (uint32_t)s.size()};
    bytes += s;
    return n;
  };
  names.push_back(add_text("id"));
  names.push_back(add_text("date"));
  names.push_back(add_text("email"));
  std::vector<Dfa> dfas;
  std::vector<std::vector<uint8_t>> nfas;
  nfa_words = 0;
  auto compile = [&](const std::string& rx, int32_t& idx) -> int {
    Dfa d;
    std::string err;
    RegexStatus st = force_nfa ? RegexStatus::TooLarge : compile_dfa(rx, d, err);
    if (st == RegexStatus::Ok) {
      idx = (int32_t)dfas.size();
      dfas.push_back(std::move(d));
      return 0;
    }
    if (st == RegexStatus::TooLarge) {
      NfaProgram np;
      err.clear();
      st = compile_nfa(rx, np, err);
      if (st == RegexStatus::Ok) {
        idx = url_nfa_code((uint32_t)nfas.size());
        nfa_words = std::max(nfa_words, np.words());
        nfas.push_back(nfa_image(np));
        return 0;
      }
    }
    if (st == RegexStatus::Syntax) return fail(OSE_EINVAL, err);
    return fail(OSE_ENOTSUP, "regexp not supported by the DFA and NFA compilers: " + err);
  };
  std::vector<UrlCustomDev> custom;
  for (auto& ci : c.custom_ids) {
    UrlCustomDev cd{};
    int rc = compile(ci.regexp, cd.dfa);
    if (rc) return rc;
    cd.name = (uint32_t)names.size();
    names.push_back(add_text(ci.template_name.empty() ? "id" : ci.template_name));
    custom.push_back(cd);
  }
  struct ParsedRule { uint32_t nseg; size_t order; std::vector<RuleSegment> segs; };
  std::vector<ParsedRule> rules;
  for (size_t k = 0; k < c.templatization_rules.size(); k++) {
    ParsedRule pr;
    std::string e = parse_user_rule(c.templatization_rules[k], pr.segs);
    if (!e.empty()) return fail(OSE_EINVAL, e);
    pr.nseg = (uint32_t)pr.segs.size();
    pr.order = k;
    rules.push_back(std::move(pr));
  }
  std::stable_sort(rules.begin(), rules.end(), [](const ParsedRule& a, const ParsedRule& b) { return a.nseg < b.nseg; });
  uint32_t longest = 0;
  for (auto& r : rules) longest = std::max(longest, r.nseg);
  // by_len[n] for n <= longest + 1 (a path with more segments than the longest rule tries none)
  std::vector<uint32_t> by_len(longest + 2, 0);
  std::vector<UrlRuleDev> rdev;
  std::vector<UrlRuleSegDev> sdev;
  uint32_t max_nseg = 0;
  for (auto& r : rules) {
    rdev.push_back(UrlRuleDev{r.nseg, (uint32_t)sdev.size()});
    max_nseg = std::max(max_nseg, r.nseg);
    for (auto& s : r.segs) {
      UrlRuleSegDev sd{};
      sd.dfa = -1;
      switch (s.kind) {
        case SegKind::Static: sd.kind = kRuleStatic; break;
        case SegKind::Wildcard: sd.kind = kRuleWildcard; break;
        case SegKind::Template: sd.kind = kRuleTemplate; break;
        case SegKind::Regex: sd.kind = kRuleRegex; break;
      }
      NameDev t = add_text(s.text);
      sd.text_off = t.off;
      sd.text_len = t.len;
      if (s.has_regexp) {
        int rc = compile(s.regexp, sd.dfa);
        if (rc) return rc;
      }
      sdev.push_back(sd);
    }
  }
  // by_len[n] = first rule with nseg >= n
  for (uint32_t n = 0; n <= longest + 1; n++) {
    uint32_t k = 0;
    while (k < rules.size() && rules[k].nseg < n) k++;
    by_len[n] = k;
  }
  max_name = 0;
  for (auto& n : names) max_name = std::max(max_name, n.len);
  h.n_custom = (uint32_t)custom.size();
  h.n_rules = (uint32_t)rdev.size();
  h.n_names = (uint32_t)names.size();
  h.n_dfa = (uint32_t)dfas.size();
  h.max_rule_nseg = max_nseg;
  h.max_name_len = max_name;
  h.rules_by_len_off = bl.put(by_len.data(), by_len.size());
  h.rules_off = bl.put(rdev.data(), rdev.size());
  h.segs_off = bl.put(sdev.data(), sdev.size());
  h.custom_off = bl.put(custom.data(), custom.size());
  h.names_off = bl.put(names.data(), names.size());
  std::vector<uint32_t> dfa_offs;
  for (auto& d : dfas) dfa_offs.push_back(put_dfa(bl, d));
  h.dfa_off = bl.put(dfa_offs.data(), dfa_offs.size());
  h.bytes_off = bl.put(bytes.data(), bytes.size());
  // the NFA programs go behind everything a config without one has, so its
  // tables are where they always were
  if (!nfas.empty()) {
    std::vector<uint32_t> nfa_offs;
    for (auto& im : nfas) nfa_offs.push_back(bl.put(im.data(), im.size()));
    h.n_nfa = (uint32_t)nfas.size();
    h.nfa_off = bl.put(nfa_offs.data(), nfa_offs.size());
  }
  bl.align();
  if (bl.overflow)
    return fail(OSE_ENOTSUP, "odigosurltemplate device tables exceed 4 GiB (the regexps' DFAs and NFA programs together)");
  bl.b.resize(bl.b.size() + 16, 0);
  h.total_bytes = (uint32_t)bl.b.size();
  std::memcpy(bl.b.data(), &h, sizeof h);
  out = std::move(bl.b);
  return 0;
}

// The URL stage's scratch for n spans, g groups of 64 and t scan tiles of 1024
// groups: the zeroed words | plan_len 4n | plan_meta 4n | plan_code 8n |
// group_sum 8g | group_base 8g | group_scr 8g | slow groups 4g | unplanned
// groups 4g | dbg | scratch (the assembled group images) | the NFA state slab.
// refs: the images go to tmpl_arena itself; an NFA engine's state slab follows.
UrlLayout url_layout(uint64_t n, uint64_t arena_bytes, uint32_t nfa_words, bool refs) {
  const size_t g = (n + kUrlGroup - 1) / kUrlGroup;
  const size_t t = (g + kUrlScanTile - 1) / kUrlScanTile;
  Carve c;
  auto part = [&](size_t bytes, size_t align = 256) { return WsPart{c.take(bytes, align), bytes}; };
  UrlLayout L;
  L.zero = part(32 + 8 * t);   // all zeroed by one memset
  L.bump = {16, 8};
  L.slow_aligned = {24, 8};
  L.scan_status = {32, 8 * t};
  L.len = part(4 * n);
  L.meta = part(4 * n, 4);
  L.code = part(8 * n, 8);
  L.gsum = part(8 * g, 8);
  L.gbase = part(8 * g, 8);
  L.gscr = part(8 * g, 8);
  L.slow = part(4 * g, 4);
  L.unpl = part(4 * g, 4);
  L.dbg = part(256);
  L.scr = part(refs ? 0 : url_scratch_bytes(n, arena_bytes));
  L.slab = nfa_words ? part(url_nfa_slab_bytes(n, nfa_words) - 256) : WsPart{c.off, 0};
  L.end = c.off;
  return L;
}

// nfa_words: 0 for an engine whose URL tables hold no NFA program
size_t url_workspace_bytes(uint64_t n, uint64_t arena_bytes, uint32_t nfa_words) {
  return url_layout(n, arena_bytes, nfa_words, false).end;
}

namespace {
// the kernels' arguments for this call, the workspace pointers from the layout
UrlKernelArgs url_args(const Engine* e, const ose_columns* c, const ose_outputs* o, uint8_t* base, const UrlLayout& L,
                       const UrlRun& r) {
  auto at = [&](const WsPart& p) { return base + p.off; };
  const uint64_t n = c->n_spans;
  const uint32_t nfa_words = e->url_words();
  UrlKernelArgs a{};
  a.n_spans = n;
  a.n_groups = (uint32_t)((n + kUrlGroup - 1) / kUrlGroup);
  a.g_begin = 0;
  a.g_end = a.n_groups;
  a.arena = c->arena;
  a.url_flags = c->url_flags;
  a.kind = c->kind;
  a.resource = c->resource;
  a.res_url_ok = c->res_url_ok;   // NULL: every resource passes (no include/exclude)
  a.path = c->path;
  a.url_out = o->url_out;
  a.tmpl = o->tmpl;
  a.out_arena = o->tmpl_arena;
  a.out_cap = o->tmpl_arena_cap;
  a.cfg = e->url_forced() ? e->url_blob_forced_dev : e->url_blob_dev;
  a.nfa = nfa_words ? 1u : 0u;
  a.nfa_words = nfa_words;
  a.nfa_slab = nfa_words ? reinterpret_cast<uint32_t*>(at(L.slab)) : nullptr;
  a.general = (!e->url.custom_ids.empty() || !e->url.templatization_rules.empty()) ? 1u : 0u;
  a.plan_len = reinterpret_cast<uint32_t*>(at(L.len));
  a.plan_meta = reinterpret_cast<uint32_t*>(at(L.meta));
  a.plan_code = reinterpret_cast<uint64_t*>(at(L.code));
  a.group_sum = reinterpret_cast<uint64_t*>(at(L.gsum));
  a.group_base = reinterpret_cast<uint64_t*>(at(L.gbase));
  a.group_scr = reinterpret_cast<uint64_t*>(at(L.gscr));
  a.scratch = at(L.scr);
  if (r.refs) {
    a.refs = 1;
    a.scratch = o->tmpl_arena;
    a.bump = reinterpret_cast<uint64_t*>(at(L.bump));
    a.slow_aligned = reinterpret_cast<uint64_t*>(at(L.slow_aligned));
  }
  a.n_scan_tiles = (uint32_t)(L.scan_status.bytes / 8);
  a.scan_counter = reinterpret_cast<uint32_t*>(base);
  a.scan_status = reinterpret_cast<uint64_t*>(at(L.scan_status));
  a.error = o->device_status ? o->device_status : reinterpret_cast<uint32_t*>(base + 8);
  a.slow_count = reinterpret_cast<uint32_t*>(base + 4);
  a.slow_groups = reinterpret_cast<uint32_t*>(at(L.slow));
  a.unplanned_count = reinterpret_cast<uint32_t*>(base + 12);
  a.unplanned = reinterpret_cast<uint32_t*>(at(L.unpl));
  a.used = o->tmpl_arena_used;
#if OSE_DIAG
  if (const char* ab = getenv("OSE_URL_ABLATE")) a.ablate = (uint32_t)strtoul(ab, nullptr, 0);   // tools/ablate_url.py
#endif
  a.plan_grid_mult = r.refs ? r.grid_mult : 1u;
  a.scr_region = (url_scratch_bytes(n, c->arena_bytes) / std::max<uint32_t>(1, url_plan_waves(a))) & ~15ull;
  // refs: image chunks of an eighth of the arena over the plan waves (at most
  // 256 KiB; a group larger than a chunk takes exactly its size): a wave
  // leaves at most one chunk's tail unused (url_refs_chunk)
  a.plan_waves = url_plan_waves(a);
  a.refs_chunk = url_refs_chunk(o->tmpl_arena_cap, a.plan_waves);
  return a;
}

// a sliced call's words: [0] the sum of the slices' unplanned counts, [1 + s]
// slice s's count: the upper half of the dbg part (the diagnostic clocks use
// the lower)
constexpr size_t kSliceWordBytes = 64;
static_assert(4 * (1 + kUrlMaxSlices) <= kSliceWordBytes, "a count word per slice and their sum");
uint32_t* url_slice_words(uint8_t* base, const UrlLayout& L) { return reinterpret_cast<uint32_t*>(base + L.dbg.off + 128); }

// fill or plan, slow plan: of the batch, or of one slice of it (url_slice_args)
int queue_url_plan(Engine* e, const UrlKernelArgs& a, hipStream_t st) {
  int rc;
  if (a.nfa) {   // every group listed as unplanned, then planned per lane
    if ((rc = e->timed("url_nfa_fill_kernel", st, [&] { launch_url_nfa_fill(a, st); }))) return rc;
    return e->timed("url_nfa_plan_kernel", st, [&] { launch_url_nfa_plan(a, st); });
  }
  if ((rc = e->timed("url_plan_kernel", st, [&] { launch_url_plan(a, st); }))) return rc;
  return e->timed("url_plan_slow_kernel", st, [&] { launch_url_plan_slow(a, st); });
}

// The plan slice by slice, each slice's event recorded behind its slow plan
// (its spans pass waits for that event alone); staggered: the odd slices on
// r.st2, which starts behind st's clears and which st waits for at the end,
// so what follows on st comes after every slice.
int queue_url_slices(Engine* e, const UrlKernelArgs& a, const UrlSlices& S, const UrlRun& r, hipStream_t st) {
  const bool two = r.form == kUrlStaggered && r.st2 && r.fork2;
  if (two) {
    HIP_TRY(hipEventRecord(r.fork2, st));
    HIP_TRY(hipStreamWaitEvent(r.st2, r.fork2, 0));
  }
  hipEvent_t last2 = nullptr;
  for (uint32_t s = 0; s < S.k; s++) {
    if (S.g[s] == S.g[s + 1]) continue;   // fewer groups than slices
    hipStream_t ss = two && (s & 1) ? r.st2 : st;
    if (const int rc = queue_url_plan(e, url_slice_args(a, S, s), ss)) return rc;
    HIP_TRY(hipEventRecord(r.slice_ev[s], ss));
    if (ss != st) last2 = r.slice_ev[s];
  }
  if (last2) HIP_TRY(hipStreamWaitEvent(st, last2, 0));
  return 0;
}

// behind the plan: scan, slow emit, and the path counts
int queue_url_rest(Engine* e, const UrlKernelArgs& a, hipStream_t st) {
  int rc;
  if ((rc = e->timed("url_scan_kernel", st, [&] { launch_url_scan(a, st); }))) return rc;
  // the groups url_plan_kernel did not assemble, written at their scanned
  // bases: nothing here reads SAMPLE's keep bytes or url_copy_kernel's
  // output, so it runs with the front (beside the trace stage when the
  // URL front has its own stream)
  rc = e->timed(a.nfa ? "url_nfa_emit_kernel" : "url_emit_slow_kernel", st, [&] {
    if (a.nfa) launch_url_nfa_emit(a, st);
    else launch_url_emit_slow(a, st);
  });
  if (rc) return rc;
  // "url_path_counts" (tests): which kernel took this call's groups, kept in
  // two spare words of the engine's path counters (ose_engine_path_counts)
  if ((e->options.load() & Engine::kOptUrlPathCounts) && e->path_count_dev) {
    // (a sliced call: the slices' lists summed by their url_plan_slow_kernel launches)
    const uint32_t* unplanned = a.unplanned_total ? a.unplanned_total : a.unplanned_count;
    HIP_TRY(hipMemcpyAsync(e->path_count_dev + 2, unplanned, 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->path_count_dev + 3, a.slow_count, 4, hipMemcpyDeviceToDevice, st));
    // word 4: the groups the NFA route took (ose_engine_url_nfa_groups)
    if (a.nfa) HIP_TRY(hipMemcpyAsync(e->path_count_dev + 4, a.unplanned_count, 4, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemsetAsync(e->path_count_dev + 4, 0, 8, st));
  }
  return 0;
}

// diagnostics (ablate & 512): the per-section shader clocks, read and printed
int print_url_clocks(const UrlKernelArgs& a, hipStream_t st) {
  uint64_t h[16];
  uint32_t cnt[4];
  HIP_TRY(hipMemcpyAsync(h, a.dbg, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(cnt, a.scan_counter, sizeof cnt, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const double wp = h[3] ? (double)h[3] : 1.0;
  fprintf(stderr, "url clocks/wave: plan[stage %.0f bitmaps %.0f plan %.0f assemble+store %.0f]\n", h[0] / wp,
          h[1] / wp, h[2] / wp, h[5] / wp);
  fprintf(stderr, "url plan list clocks/wave: enumerate %.0f classify %.0f fold %.0f\n", h[13] / wp, h[14] / wp,
          h[15] / wp);
  fprintf(stderr, "url groups: %llu, slow (K3s) %u, unplanned (K1b) %u\n", (unsigned long long)((a.n_spans + 63) / 64),
          cnt[1], cnt[3]);
  fprintf(stderr, "url_plan_slow_kernel slowest block clocks: config %llu whole %llu plan_path %llu\n",
          (unsigned long long)h[8], (unsigned long long)h[9], (unsigned long long)h[10]);
  return 0;
}
}  // namespace

int run_url(Engine* e, const ose_columns* c, const ose_outputs* o, hipStream_t st, Workspace* ws, const UrlRun& r,
            UrlKernelArgs* front) {
  if (!e->has_url) return fail(OSE_EINVAL, "odigosurltemplate is not configured on this engine");
  if (!c->url_flags || !c->kind || !c->path || !c->arena || !o->url_out || !o->tmpl || !o->tmpl_arena)
    return fail(OSE_EINVAL, "TEMPLATE stage needs url_flags, kind, path, arena, url_out, tmpl, tmpl_arena");
  if (e->url_needs_resource && (!c->resource || !c->res_url_ok))
    return fail(OSE_EINVAL, "include/exclude configured: resource and res_url_ok columns are required");
  if (c->res_url_ok && !c->resource) return fail(OSE_EINVAL, "res_url_ok needs the resource column");
  if (o->tmpl_arena_cap > 0xFFFFFFFFull) return fail(OSE_ERANGE, "tmpl_arena_cap exceeds the 32-bit offset range");
  const UrlLayout L = url_layout(c->n_spans, c->arena_bytes, e->url_words(), r.refs);
  int rc = ws->reserve(r.ws_off + L.end);
  if (rc) return rc;
  uint8_t* base = static_cast<uint8_t*>(ws->dev) + r.ws_off;
  HIP_TRY(hipMemsetAsync(base, 0, L.zero.bytes, st));
  UrlKernelArgs a = url_args(e, c, o, base, L, r);
  *front = a;
  if (a.n_spans == 0) {
    if (o->tmpl_arena_used) HIP_TRY(hipMemsetAsync(o->tmpl_arena_used, 0, 8, st));
    if (r.planned) HIP_TRY(hipEventRecord(r.planned, st));
    return 0;
  }
  if (a.ablate & 512) {   // diagnostics: per-section shader clocks (tools/url_clocks.py)
    a.dbg = reinterpret_cast<uint64_t*>(base + L.dbg.off);
    HIP_TRY(hipMemsetAsync(a.dbg, 0, 256, st));
  }
  if (r.slices > 1 && r.refs && !a.nfa && r.slice_ev) {
    // the slices' count words and their sum (cleared by clear_url_slice_words);
    // one image chunk size for the plan waves of all slices together, so the
    // arena's unused chunk tails stay under an eighth of it whatever K is
    const UrlSlices S = url_slices(a.n_groups, r.slices, r.form);
    a.unplanned_total = url_slice_words(base, L);
    uint32_t waves = 0;
    for (uint32_t s = 0; s < S.k; s++)
      if (S.g[s] < S.g[s + 1]) waves += url_plan_waves(url_slice_args(a, S, s));
    a.plan_waves = waves;
    a.refs_chunk = url_refs_chunk(o->tmpl_arena_cap, waves);
    *front = a;
    rc = queue_url_slices(e, a, S, r, st);
  } else {
    rc = queue_url_plan(e, a, st);
    if (!rc && r.planned) HIP_TRY(hipEventRecord(r.planned, st));
  }
  if (!rc) rc = queue_url_rest(e, a, st);
  if (!rc) *front = a;
  return rc;
}

UrlKernelArgs url_slice_args(const UrlKernelArgs& a, const UrlSlices& S, uint32_t s) {
  UrlKernelArgs x = a;
  x.g_begin = S.g[s];
  x.g_end = S.g[s + 1];
  x.plan_grid_mult = url_plan_grid_mult(x.g_end - x.g_begin, true);   // a wave keeps its ~19 groups
  x.unplanned = a.unplanned + x.g_begin;
  x.unplanned_count = a.unplanned_total + 1 + s;
  x.copy_blocks = S.part[s + 1] - S.part[s];
  x.partial_off = S.part[s];
  return x;
}

// The slices' count words cleared on the caller's stream ahead of the fork:
// on the side stream the fill would be queued as the trace stage's grid
// starts, where a fill was measured starved (285 us for these 64 bytes,
// profiles/tail_slices_ab.txt), and the zeroed part of the layout has no
// room for them.
int clear_url_slice_words(Engine* e, const ose_columns* c, Workspace* ws, size_t ws_off, hipStream_t st) {
  const UrlLayout L = url_layout(c->n_spans, c->arena_bytes, e->url_words(), true);
  if (const int rc = ws->reserve(ws_off + L.end)) return rc;
  HIP_TRY(hipMemsetAsync(url_slice_words(static_cast<uint8_t*>(ws->dev) + ws_off, L), 0, kSliceWordBytes, st));
  return 0;
}

int run_url_back_slice(Engine* e, const UrlKernelArgs& a, const UrlSlices& S, uint32_t s, hipStream_t st) {
  if (S.g[s] == S.g[s + 1] || !a.fuse_size) return 0;
  const UrlKernelArgs x = url_slice_args(a, S, s);
  return e->timed("url_copy_kernel", st, [&] { launch_url_copy(x, st); });
}

int run_url_back(Engine* e, const UrlKernelArgs& a, hipStream_t st) {
  if (a.n_spans == 0) return 0;
  // refs form: every span's ref is written by the kernel that placed its
  // group, so url_copy_kernel runs only as the fused spans pass
  if (!a.refs || a.fuse_size)
    if (const int rc = e->timed("url_copy_kernel", st, [&] { launch_url_copy(a, st); })) return rc;
  return (a.ablate & 512) ? print_url_clocks(a, st) : 0;
}

}  // namespace ose

using namespace ose;

// Diagnostic, no device: the URL stage's workspace, part by part in
// UrlLayout's order, and url_workspace_bytes for the same batch; returns the
// number of parts.
extern "C" uint32_t osehost_url_layout(uint64_t n_spans, uint64_t arena_bytes, uint32_t nfa_words, int refs, uint64_t* off,
                                       uint64_t* bytes, uint32_t cap, uint64_t* end, uint64_t* workspace_bytes) {
  if (workspace_bytes) *workspace_bytes = url_workspace_bytes(n_spans, arena_bytes, nfa_words);
  return layout_parts(url_layout(n_spans, arena_bytes, nfa_words, refs != 0), off, bytes, cap, end);
}

// Diagnostic, no device: the slices of a sliced call (kernels.hpp url_slices),
// K = 0: url_tail_slices()'s rule and form.  out[0] = the slices, out[1] = the
// kept partials the size scratch reserves, out[2..11) the group bounds,
// out[11..20) the partial offsets (entries past the slices' repeat the end).
extern "C" void osehost_url_slices(uint32_t n_groups, uint32_t k, uint32_t form, uint32_t* out) {
  if (k == 0) {
    k = url_tail_slices(n_groups);
    form = kUrlTailForm;
  }
  const UrlSlices S = url_slices(n_groups, k, form);
  out[0] = S.k;
  out[1] = size_partials_cap();
  for (uint32_t j = 0; j <= kUrlMaxSlices; j++) {
    out[2 + j] = S.g[j < S.k ? j : S.k];
    out[3 + kUrlMaxSlices + j] = S.part[j < S.k ? j : S.k];
  }
}

// FNV-1a of the odigosurltemplate device tables of an engine config, their
// size and the number of NFA programs in them, for tests that pin the tables
// of a config without an NFA program.  No device is touched.
extern "C" int osehost_url_blob_hash(const char* cfg_json, int force_nfa, uint64_t* hash, uint64_t* bytes,
                                     uint32_t* n_nfa) {
  Json root;
  try {
    root = parse_json(cfg_json ? cfg_json : "{}");
  } catch (const std::exception& ex) {
    return fail(OSE_EINVAL, ex.what());
  }
  const Json* j = root.is_obj() ? root.get("odigosurltemplate") : nullptr;
  if (!j) return fail(OSE_EINVAL, "odigosurltemplate is not configured");
  UrlTemplateConfig url;
  const std::string err = decode_url_config(*j, url);
  if (!err.empty()) return fail(OSE_EINVAL, err);
  std::vector<uint8_t> blob;
  uint32_t max_name = 0, words = 0;
  if (const int rc = build_url_blob(url, blob, max_name, force_nfa != 0, words)) return rc;
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint8_t b : blob) h = (h ^ b) * 0x100000001b3ull;
  if (hash) *hash = h;
  if (bytes) *bytes = blob.size();
  if (n_nfa) *n_nfa = reinterpret_cast<const UrlCfgDev*>(blob.data())->n_nfa;
  return 0;
}
