// otlp_host.cpp — OTLP protobuf ingest: ose_otlp_decode, the
// batch's accessors and its release.  The batch type is in otlp_batch.hpp; the
// way back to bytes (ose_otlp_encode*) is otlp_encode_host.cpp, the engine
// option otlp_condattr's columns are otlp_condattr_host.cpp.  Every device
// slab is laid out by slab.hpp's carver.
//
// One call turns a serialized TracesData into device columns; decode() is
// these steps, a function each:
//   1. upload_message: the bytes go to pinned staging and H2D (the arena:
//      strings are referenced in place);
//   2. walk_records, walk_scopes: meanwhile the structure is walked
//      (ResourceSpans / ScopeSpans headers, resource and scope contents, one
//      header per span) by the host (walk: otlp_pb.cpp's reader, the resources'
//      and scopes' columns from columnize.cpp) or, below the TracesData chain,
//      on the GPU (res_walk_gpu, scope_walk_gpu); column_slab lays the device
//      columns out and uploads the host's;
//   3. span_kernels: otlp_span_kernel decodes every span on the GPU; under the
//      engine option otlp_sqlop, otlp_sqlop_kernel then reads db.query.text /
//      db.operation.name (db_flags, db_query) and may add spans to the list;
//      under otlp_condattr, otlp_condattr_kernel reads the first KeyValue of
//      each odigosconditionalattributes key (ose_otlp_condattr_columns) and may
//      add spans too; under otlp_url_full, otlp_url_full_kernel last parses the
//      url.full / http.url of the spans whose path has no other source
//      (url_full.hpp), and a scan places the paths that hold escapes;
//   4. host_pass: the spans they list get pb_span + columnize_span, their
//      strings appended after the message bytes (regrow_arena), written by
//      otlp_fix_kernel (and otlp_sqlop_fix_kernel); under otlp_condattr that
//      stage's entries of the listed spans and its per-scope and per-resource
//      columns are then made on the host (condattr_finish).  Between the two,
//      url_full_unescape writes the unescaped url.full paths behind the host
//      pass's strings.
#include <algorithm>
#include <chrono>
#include <deque>
#include <shared_mutex>
#include <cstring>
#include <map>
#include <string_view>
#include <thread>
#include <unordered_map>

#include "columnize.hpp"
#include "engine_internal.hpp"
#include "kernels.hpp"
#include "otlp_batch.hpp"
#include "otlp_encode.hpp"
#include "otlp_pb.hpp"
#include "taskpool.hpp"
#include "url_full.hpp"

namespace ose {

int DevBuf::need(size_t bytes) {
  if (bytes <= cap) return 0;
  if (p) { if (host) (void)hipHostFree(p); else (void)hipFree(p); }
  p = nullptr;
  cap = 0;
  const size_t want = up(std::max<size_t>(bytes + bytes / 4, 1 << 20), 1 << 16);
  if (host) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p), want, hipHostMallocDefault));
  else HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), want));
  cap = want;
  return 0;
}

namespace {
struct CachedRes {
  uint32_t svc, svc_str, set, rpart;   // set: id in ResCache::sets
  uint8_t ok;
  uint64_t attr_res;
  uint8_t sql_ok;   // !shouldExcludeLanguage (1 on an engine without odigossqldboperationprocessor)
};

// Resource columns by message bytes, kept across calls (a gateway sees the
// same pods' resources batch after batch), and the attribute sets interned.
struct ResCache {
  static constexpr size_t kMaxEntries = size_t(1) << 16;
  std::shared_mutex mu;
  std::deque<std::string> keys;   // owned bytes the map's views point into
  std::unordered_map<std::string_view, CachedRes> map;
  std::deque<std::vector<std::pair<std::string, std::string>>> sets;   // stable addresses
  std::map<std::vector<std::pair<std::string, std::string>>, uint32_t> set_ids;
  uint32_t intern(const std::vector<std::pair<std::string, std::string>>& set) {   // under the unique lock
    auto it = set_ids.find(set);
    if (it != set_ids.end()) return it->second;
    const uint32_t id = (uint32_t)sets.size();
    sets.push_back(set);
    set_ids.emplace(set, id);
    return id;
  }
};
}  // namespace

// The engine's view for the ingest: the columniser context and the key
// table the GPU decoder matches (built once per engine).
// The device copy of the resource cache (ResCache) the GPU ResourceSpans
// pass looks resources up in (otlp_res_fields_kernel): open addressing on
// the Resource bytes' FNV-1a hash, up to 64 probes, never deleted.  A host
// mirror takes the inserts; sync() copies what changed.  Lookups in flight
// hold the lock shared, updates unique.
struct DevResTable {
  std::shared_mutex mu;
  ResSlotDev* d_slots = nullptr;
  uint8_t* d_keys = nullptr;
  std::vector<ResSlotDev> slots;
  std::vector<uint8_t> keys;
  std::vector<uint32_t> changed;   // slots filled since the last sync
  size_t keys_synced = 0;
  uint32_t n = 0;
  int ensure() {   // under the unique lock
    if (d_slots) return 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_slots), sizeof(ResSlotDev) * kResSlots));
    HIP_TRY(hipMemset(d_slots, 0, sizeof(ResSlotDev) * kResSlots));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_keys), kResKeyBytes));
    slots.assign(kResSlots, ResSlotDev{});
    return 0;
  }
  void insert(const uint8_t* key, uint32_t len, const CachedRes& cr) {   // under the unique lock
    if (!d_slots || n >= kResSlots / 2 || keys.size() + len > kResKeyBytes) return;
    uint64_t h = kResHashSeed;
    for (uint32_t q = 0; q < len; q++) h = res_key_hash_step(h, key[q]);
    uint32_t slot = (uint32_t)h & (kResSlots - 1);
    for (int probe = 0; probe < 64; probe++, slot = (slot + 1) & (kResSlots - 1)) {
      ResSlotDev& e = slots[slot];
      if (!e.ready) {
        e.h = h;
        e.koff = (uint32_t)keys.size();
        e.klen = len;
        keys.insert(keys.end(), key, key + len);
        e.svc = cr.svc;
        e.svc_str = cr.svc_str;
        e.set = cr.set;
        e.rpart = cr.rpart;
        e.attr_res = cr.attr_res;
        e.ok = (uint32_t)cr.ok | ((uint32_t)cr.sql_ok << 1);
        e.ready = 1;
        changed.push_back(slot);
        n++;
        return;
      }
      if (e.h == h && e.klen == len && std::memcmp(keys.data() + e.koff, key, len) == 0) return;
    }
  }
  int sync(hipStream_t st) {   // under the unique lock
    if (changed.empty()) return 0;
    if (keys.size() > keys_synced)
      HIP_TRY(hipMemcpyAsync(d_keys + keys_synced, keys.data() + keys_synced, keys.size() - keys_synced,
                             hipMemcpyHostToDevice, st));
    if (changed.size() > 256) {
      HIP_TRY(hipMemcpyAsync(d_slots, slots.data(), sizeof(ResSlotDev) * kResSlots, hipMemcpyHostToDevice, st));
    } else {
      for (uint32_t k : changed)
        HIP_TRY(hipMemcpyAsync(d_slots + k, &slots[k], sizeof(ResSlotDev), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));   // the sources are the mirror, which the next insert changes
    keys_synced = keys.size();
    changed.clear();
    return 0;
  }
  ~DevResTable() {
    if (d_slots) (void)hipFree(d_slots);
    if (d_keys) (void)hipFree(d_keys);
  }
};

struct OtlpEngine {
  ColumnizeCtx ctx;
  std::vector<OtlpKeyDev> keys;
  std::string key_bytes;
  uint64_t key_lens = 0;
  uint8_t* keys_dev = nullptr;   // OtlpKeyDev[] then the bytes
  uint32_t n_attr_keys = 0;
  uint32_t attr_words = 1;   // attr_match words per span
  bool json_rules = false;
  // more than 64 shim-evaluated (json / oversize-regex) span_attribute rules:
  // the per-resource cached word cannot hold their bits, so the host pass
  // takes each span's from its resource's service id (AsString(service.name):
  // the rules whose service it is, spanattribute.go:130-132), [svc][word]
  bool wide_host_rules = false;
  std::vector<std::vector<uint64_t>> host_rules_by_svc;
  ResCache res_cache;
  DevResTable res_dev;
  std::string err;
  ~OtlpEngine() { if (keys_dev) (void)hipFree(keys_dev); }
};

namespace {
std::mutex g_otlp_mu;

OtlpEngine* otlp_engine(Engine* e, int& rc) {
  std::lock_guard<std::mutex> g(g_otlp_mu);
  rc = 0;
  if (e->otlp) return e->otlp;
  auto* o = new OtlpEngine();
  o->err = o->ctx.build(e->has_url ? &e->url : nullptr, e->has_sampling ? &e->sampling : nullptr,
                        e->has_traffic ? &e->traffic : nullptr, e->has_sqlop ? &e->sqlop : nullptr);
  if (!o->err.empty()) { rc = fail(OSE_EINVAL, o->err); delete o; return nullptr; }
  std::map<std::string, uint64_t> roles;
  roles["http.request.method"] |= kRoleMethodNew;
  roles["http.method"] |= kRoleMethodOld;
  roles["http.route"] |= kRoleRoute;
  roles["url.template"] |= kRoleUrlTmpl;
  roles["url.path"] |= kRoleUrlPath;
  roles["http.target"] |= kRoleTarget;
  roles["url.full"] |= kRoleFull;
  roles["http.url"] |= kRoleFull;
  const AttrPlan& plan = o->ctx.attr_plan;
  // the per-resource rule word the decoder caches holds the shim-evaluated
  // rules only, one bit each; past 64 of them the host pass takes the bits
  // from the resource's service id instead (wide_host_rules)
  size_t n_host_rules = 0;
  for (int rk : plan.rule_key) n_host_rules += rk < 0;
  if (n_host_rules > 64) {
    o->wide_host_rules = true;
    o->host_rules_by_svc.assign(std::max<size_t>(o->ctx.services.size(), 1),
                                std::vector<uint64_t>(std::max<size_t>(plan.host_mask.size(), 1), 0));
    for (size_t k = 0; k < plan.rule_key.size() && k < o->ctx.attr_preds.size(); k++) {
      if (plan.rule_key[k] >= 0) continue;
      auto it = o->ctx.services.find(o->ctx.attr_preds[k].service());
      if (it != o->ctx.services.end() && it->second < o->host_rules_by_svc.size())
        o->host_rules_by_svc[it->second][k / 64] |= 1ull << (k % 64);
    }
  }
  o->attr_words = (uint32_t)std::max<size_t>(1, (plan.rule_key.size() + 63) / 64);
  o->n_attr_keys = (uint32_t)plan.keys.size();
  // key columns past kOtlpMaxAttrKeys have no role bit: a span that carries
  // such a key takes the host pass (which fills every key column), and the
  // GPU decoder writes the others ABSENT for every span it finishes
  for (size_t k = 0; k < plan.keys.size(); k++)
    roles[plan.keys[k]] |= k < kOtlpMaxAttrKeys ? kRoleAttr0 << k : (uint64_t)kRoleHost;
  for (size_t k = 0; k < plan.rule_key.size(); k++)
    if (plan.rule_key[k] < 0) {
      roles[o->ctx.attr_preds[k].key()] |= kRoleHost;
      o->json_rules = true;
    }
  for (auto& kv : roles) {
    OtlpKeyDev d{(uint32_t)kv.first.size(), (uint32_t)o->key_bytes.size(), kv.second};
    o->key_bytes += kv.first;
    o->keys.push_back(d);
    o->key_lens |= 1ull << std::min<size_t>(kv.first.size(), 63);   // bit 63: every length >= 63
  }
  const size_t kb = o->keys.size() * sizeof(OtlpKeyDev);
  std::vector<uint8_t> blob(kb + o->key_bytes.size() + 16, 0);
  std::memcpy(blob.data(), o->keys.data(), kb);
  std::memcpy(blob.data() + kb, o->key_bytes.data(), o->key_bytes.size());
  if (hipMalloc(reinterpret_cast<void**>(&o->keys_dev), blob.size()) != hipSuccess ||
      hipMemcpy(o->keys_dev, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
    rc = fail(OSE_EDEVICE, "OTLP ingest: key table upload failed");
    delete o;
    return nullptr;
  }
  e->otlp = o;
  return o;
}
}  // namespace

void release_otlp(Engine* e) {
  for (void* p : e->otlp_pool) delete static_cast<OtlpBatchImpl*>(p);
  e->otlp_pool.clear();
  delete e->otlp;
  e->otlp = nullptr;
}

namespace {
// memcpy over threads for large copies into pinned staging
void par_memcpy(uint8_t* dst, const uint8_t* src, size_t n) {
  const size_t kChunk = size_t(64) << 20;
  if (n < 2 * kChunk) { std::memcpy(dst, src, n); return; }
  const int T = (int)std::min<size_t>(16, n / kChunk);
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++)
    th.emplace_back([=]() { const size_t a = n * t / T, b = n * (t + 1) / T; std::memcpy(dst + a, src + a, b - a); });
  std::memcpy(dst, src, n / T);
  for (auto& x : th) x.join();
}

// The structural walk, resources split over threads.  Resource and scope
// messages repeat across a batch (one SDK, one pod), so their columns are
// cached by message bytes.
struct Walked {
  std::vector<uint64_t> span_ref;   // with gpu_scopes: the host-walked scopes' spans only
  std::vector<uint8_t> scope_on_host;
  std::vector<uint32_t> scope_count;
  std::vector<uint32_t> span_res, span_scope;
  std::vector<uint32_t> res_svc, res_svc_str, res_attrset, res_size, scope_size, scope_res;
  std::vector<uint8_t> res_ok, res_sql_ok;
  std::vector<uint64_t> attr_res;
  std::vector<std::vector<std::pair<std::string, std::string>>> sets;
  OtlpLayout lay;   // what the re-encoder needs (otlp_encode.cpp)
  std::string err;
};
struct WalkChunk {
  std::vector<uint64_t> span_ref;
  std::vector<uint32_t> span_res, span_scope;   // chunk-local indices
  std::vector<uint32_t> res_svc, res_svc_str, res_set, res_size, scope_size, scope_res;
  std::vector<uint8_t> res_ok, res_sql_ok;
  std::vector<uint64_t> attr_res;
  OtlpLayout lay;   // res_scope0 / scope_span0 chunk-local
  // GPU-walked scopes (walk with gpu_scopes): span_ref lists only the spans
  // of the scopes the host walked
  std::vector<uint8_t> scope_on_host;
  std::vector<uint32_t> scope_count;
  std::string err;
};
// ScopeSpans payloads up to this size are walked on the GPU (a lane per
// scope follows its chain of span lengths); larger ones on the host
constexpr size_t kGpuScopeBytes = size_t(64) << 10;
uint64_t sov64(uint64_t x) { uint64_t n = 1; while (x >= 0x80) { x >>= 7; n++; } return n; }
uint64_t flen(uint64_t l) { return 1 + sov64(l) + l; }

// The json (host-pass) span_attribute rules of a resource as one word: bit j
// for the j-th host rule in rule order (words: the resource's bits of every
// rule, 64 per word; ColumnizeCtx::attr_plan.host_mask marks the host rules)
uint64_t host_rule_word(const AttrPlan& p, const std::vector<uint64_t>& words) {
  uint64_t out = 0;
  uint32_t j = 0;
  for (size_t w = 0; w < p.host_mask.size(); w++)
    for (uint64_t m = p.host_mask[w]; m; m &= m - 1, j++)
      if (j < 64 && w < words.size() && ((words[w] >> __builtin_ctzll(m)) & 1)) out |= 1ull << j;
  return out;
}
// ... and back to the rule-indexed words columnize_span takes
void host_rule_words(const AttrPlan& p, uint64_t word, std::vector<uint64_t>& out) {
  out.assign(std::max<size_t>(1, p.host_mask.size()), 0);
  uint32_t j = 0;
  for (size_t w = 0; w < p.host_mask.size(); w++)
    for (uint64_t m = p.host_mask[w]; m; m &= m - 1, j++)
      if (j < 64 && ((word >> j) & 1)) out[w] |= 1ull << __builtin_ctzll(m);
}

// A resource's columns from its Resource field(s) (merged as pdata merges
// them), entered into the cache by message bytes when there is at most one
// field.  False: a malformed Resource.
using FieldRefs = std::vector<std::pair<size_t, size_t>>;   // (offset in the message, length)
std::string_view res_key(const uint8_t* p, const FieldRefs& resf) {   // the cache key: the one Resource field's bytes
  return resf.size() == 1 ? std::string_view((const char*)p + resf[0].first, resf[0].second) : std::string_view();
}
bool resolve_resource(const ColumnizeCtx& ctx, ResCache& cache, const uint8_t* p, const FieldRefs& resf,
                      ProtoSizer& sizer, CachedRes& cr) {
  AttrMap attrs;
  uint32_t dropped = 0;
  for (auto& x : resf)
    if (!pb_resource(p + x.first, x.second, attrs, dropped)) return false;
  const ResourceCols rc = columnize_resource(ctx, attrs);
  cr.svc = rc.svc;
  cr.svc_str = rc.svc_str;
  cr.ok = rc.url_ok;
  cr.sql_ok = rc.sql_ok;
  cr.attr_res = host_rule_word(ctx.attr_plan, rc.attr_res);   // <= 64 json rules (otlp_engine)
  cr.rpart = (uint32_t)flen(sizer.attrs(attrs, 1) + (dropped ? 1 + sov64(dropped) : 0));   // Resource: always emitted
  const std::string_view key = res_key(p, resf);
  std::unique_lock<std::shared_mutex> g(cache.mu);
  cr.set = cache.intern(rc.attrset);
  if (resf.size() <= 1 && cache.map.size() < ResCache::kMaxEntries && !cache.map.count(key)) {
    cache.keys.emplace_back(key);
    cache.map.emplace(std::string_view(cache.keys.back()), cr);
  }
  return true;
}

// ... from the cache (looked up under the shared lock) when there is at most
// one Resource field, else resolved
bool cached_resource(const ColumnizeCtx& ctx, ResCache& cache, const uint8_t* p, const FieldRefs& resf,
                     ProtoSizer& sizer, CachedRes& cr) {
  if (resf.size() <= 1) {
    std::shared_lock<std::shared_mutex> g(cache.mu);
    auto ci = cache.map.find(res_key(p, resf));
    if (ci != cache.map.end()) {
      cr = ci->second;
      return true;
    }
  }
  return resolve_resource(ctx, cache, p, resf, sizer, cr);
}

// The fields of the ResourceSpans record at [ro, ro + rl): the Resource
// field(s) into resf and, where asked for, the ScopeSpans (2), the deprecated
// ones (1000) and the schema_url's length.  False: a malformed record (fields
// 1 / 2 / 3 / 1000 must be length-delimited).
bool res_record_fields(const uint8_t* p, size_t ro, size_t rl, FieldRefs& resf, FieldRefs* scopes = nullptr,
                       FieldRefs* deprecated = nullptr, size_t* schema = nullptr) {
  PbReader rr(p + ro, rl);
  resf.clear();
  uint32_t f, wt;
  while (rr.more() && rr.tag(f, wt)) {
    size_t o, l;
    if (f == 1 || f == 2 || f == 1000 || f == 3) {
      if (wt != 2 || !rr.bytes(o, l)) { rr.fail(); break; }
      if (f == 1) resf.emplace_back(ro + o, l);
      else if (f == 3) { if (schema) *schema = l; }
      else if (scopes) (f == 2 ? scopes : deprecated)->emplace_back(ro + o, l);
    } else {
      rr.skip(wt, f);
    }
  }
  return rr.ok;
}

// The TracesData records that start in [s, lim) (a record may run past lim:
// *end is where the last one ends), each ResourceSpans walked in full.
void walk_segment(const ColumnizeCtx& ctx, ResCache& cache, const uint8_t* p, size_t n, size_t s, size_t lim,
                  WalkChunk& c, size_t* end, bool gpu_scopes, bool chain = false) {
  std::unordered_map<std::string_view, CachedRes> rcache;   // this call's, by view into the message
  std::unordered_map<std::string_view, uint32_t> scache;
  ProtoSizer sizer;
  std::vector<std::pair<size_t, size_t>> resf, scopes, deprecated, scf;
  const size_t est = gpu_scopes ? 16 : (std::min(lim, n) - std::min(s, n)) / 128 + 16;   // spans of >= 128 bytes
  c.span_ref.reserve(est);
  c.span_res.reserve(est);
  c.span_scope.reserve(est);
  PbReader top(p, n);
  top.i = s;
  *end = s;
  // The walk is a chain of lengths: each header's address depends on the
  // last length, so without help every span costs a DRAM round trip.  The
  // segment is prefetched line by line a few KB ahead of the walk instead.
  size_t pf = s & ~size_t(63);
  auto ahead = [&](size_t pos) {
    if (gpu_scopes) return;   // the host reads headers only: no streaming of span bytes
    const size_t want = std::min(n, pos + 8192);
    for (; pf < want; pf += 64) __builtin_prefetch(p + pf, 0, 3);
  };
  uint32_t tf, twt;
  while (top.i < lim && top.more() && top.tag(tf, twt)) {
    ahead(top.i);
    size_t ro, rl;
    if (tf != 1) {
      if (!top.skip(twt, tf)) break;
      *end = top.i;
      continue;
    }
    if (twt != 2 || !top.bytes(ro, rl)) { top.fail(); break; }
    *end = top.i;
    if (gpu_scopes && top.i + 2 < n) __builtin_prefetch(p + top.i, 0, 3);   // the next record's header
    if (chain) {   // the TracesData chain only: the GPU walks each record (otlp_res_fields_kernel)
      if (ro > 0xFFFFFFFFull || rl > 0xFFFFFFFFull) { c.err = "ResourceSpans beyond the 4 GiB arena range"; return; }
      c.lay.res_ref.push_back(ro | ((uint64_t)rl << 32));
      continue;
    }
    scopes.clear();
    deprecated.clear();
    size_t schema = 0;
    uint32_t f, wt;
    if (!res_record_fields(p, ro, rl, resf, &scopes, &deprecated, &schema)) {
      c.err = "OTLP protobuf: malformed ResourceSpans";
      return;
    }
    if (scopes.empty()) scopes.swap(deprecated);
    // the resource's columns (cached by its message bytes: this call's cache first)
    CachedRes cr{};
    const std::string_view key = res_key(p, resf);
    auto it = resf.size() <= 1 ? rcache.find(key) : rcache.end();
    if (it != rcache.end()) {
      cr = it->second;
    } else {
      if (!cached_resource(ctx, cache, p, resf, sizer, cr)) { c.err = "OTLP protobuf: malformed Resource"; return; }
      if (resf.size() <= 1) rcache.emplace(key, cr);
    }
    const uint32_t rloc = (uint32_t)c.res_svc.size();
    c.lay.res_ref.push_back(ro | ((uint64_t)rl << 32));
    c.lay.res_scope0.push_back((uint32_t)c.scope_size.size());
    c.res_svc.push_back(cr.svc);
    c.res_svc_str.push_back(cr.svc_str);
    c.res_ok.push_back(cr.ok);
    c.res_sql_ok.push_back(cr.sql_ok);
    c.attr_res.push_back(cr.attr_res);
    c.res_set.push_back(cr.set);
    c.res_size.push_back(cr.rpart + (uint32_t)(schema ? flen(schema) : 0));
    for (auto& so : scopes) {
      const uint32_t sloc = (uint32_t)c.scope_size.size();
      PbReader sr(p + so.first, so.second);
      size_t sschema = 0, sschema_off = 0;
      scf.clear();
      c.lay.scope_ref.push_back(so.first | ((uint64_t)so.second << 32));
      c.lay.scope_span0.push_back((uint32_t)c.span_ref.size());
      if (gpu_scopes && so.second <= kGpuScopeBytes) {   // counted, sized and listed on the GPU
        c.scope_on_host.push_back(0);
        c.scope_count.push_back(0);
        c.scope_size.push_back(0);
        c.scope_res.push_back(rloc);
        c.lay.scope_hdr.push_back(0);
        c.lay.scope_schema.push_back(0);
        continue;
      }
      const size_t first_span = c.span_ref.size();
      while (sr.more() && sr.tag(f, wt)) {
        size_t o, l;
        if (f == 1 || f == 2 || f == 3) {
          if (wt != 2 || !sr.bytes(o, l)) { sr.fail(); break; }
          if (f == 1) {
            scf.emplace_back(so.first + o, l);
          } else if (f == 3) {
            sschema = l;
            sschema_off = so.first + o;
          } else {
            const uint64_t off = so.first + o;
            ahead(off + l);
            if (off > 0xFFFFFFFFull || l > 0xFFFFFFFFull) { c.err = "span beyond the 4 GiB arena range"; return; }
            c.span_ref.push_back(off | ((uint64_t)l << 32));
            if (!gpu_scopes) {
              c.span_res.push_back(rloc);
              c.span_scope.push_back(sloc);
            }
          }
        } else {
          sr.skip(wt, f);
        }
      }
      if (!sr.ok) { c.err = "OTLP protobuf: malformed ScopeSpans"; return; }
      uint32_t spart;
      const std::string_view sk = scf.size() == 1 ? std::string_view((const char*)p + scf[0].first, scf[0].second)
                                                  : std::string_view();
      auto si = scf.size() <= 1 ? scache.find(sk) : scache.end();
      if (si != scache.end()) {
        spart = si->second;
      } else {
        ScopeSpans meta;
        for (auto& x : scf)
          if (!pb_scope(p + x.first, x.second, meta)) { c.err = "OTLP protobuf: malformed InstrumentationScope"; return; }
        spart = (uint32_t)sizer.scope_fixed(meta);   // schema_url empty here
        if (scf.size() <= 1) scache.emplace(sk, spart);
      }
      c.scope_size.push_back(spart + (uint32_t)(sschema ? flen(sschema) : 0));
      c.scope_res.push_back(rloc);
      c.lay.scope_hdr.push_back(scf.empty() ? 0
                                : scf.size() == 1 ? (scf[0].first | ((uint64_t)scf[0].second << 32))
                                                  : OtlpLayout::kMulti);
      c.lay.scope_schema.push_back(sschema_off | ((uint64_t)sschema << 32));
      c.scope_on_host.push_back(1);
      c.scope_count.push_back((uint32_t)(c.span_ref.size() - first_span));
    }
  }
  if (!top.ok) c.err = "OTLP protobuf: malformed TracesData";
}

// A plausible record start at or after k: a TracesData field 1 (0x0A) whose
// length varint frames a record followed by 3 more such records (or the end).
size_t find_start(const uint8_t* p, size_t n, size_t k) {
  for (size_t q = k; q + 2 < n; q++) {
    if (p[q] != 0x0A) continue;
    size_t pos = q;
    int hops = 0;
    bool ok = true;
    while (hops < 4 && pos < n) {
      PbReader r(p, n);
      r.i = pos;
      uint32_t f, wt;
      size_t o, l;
      if (!r.tag(f, wt) || f != 1 || wt != 2 || !r.bytes(o, l) || l == 0 || (p[o] != 0x0A && p[o] != 0x12)) {
        ok = false;
        break;
      }
      pos = r.i;
      hops++;
    }
    if (ok) return q;
  }
  return n;
}

// The segments walked over threads (chain: walk_segment's TracesData chain
// alone): the records form one chain of lengths, so each thread starts at a
// speculated record start and walks up to the next thread's; the split is
// exact iff every thread ends exactly where the next one started (the chain
// from 0 is unique), else the walk runs again on one thread.
bool walk_split(const ColumnizeCtx& ctx, ResCache& cache, const uint8_t* p, size_t n, bool gpu_scopes, bool chain,
                std::vector<WalkChunk>& ch, std::string& err) {
  const size_t kSeg = size_t(256) << 10;
  int T = (int)std::max<size_t>(1, std::min<size_t>({(size_t)parallel_width(), n / kSeg}));
#if OSE_DIAG
  if (const char* e = getenv("OSE_WALK_THREADS")) T = std::max(1, atoi(e));
#endif
  for (int attempt = 0; attempt < 2; attempt++) {
    if (attempt) T = 1;
    std::vector<size_t> st((size_t)T + 1, n), en((size_t)T, 0);
    st[0] = 0;
    for (int t = 1; t < T; t++) st[t] = find_start(p, n, n * (size_t)t / (size_t)T);
    for (int t = T - 1; t >= 1; t--) st[t] = std::min(st[t], st[t + 1]);   // monotone
    ch.assign((size_t)T, WalkChunk());
    parallel_run(T, [&](int t) { walk_segment(ctx, cache, p, n, st[t], st[t + 1], ch[t], &en[t], gpu_scopes, chain); });
    bool exact = true;
    for (int t = 0; t < T; t++) {
      if (!ch[t].err.empty()) {
        if (t == 0 || attempt) { err = ch[t].err; return false; }
        exact = false;   // a speculated start inside a record: redo
      }
      if (t + 1 < T && en[t] != st[t + 1]) exact = false;
    }
    if (en[T - 1] != n && ch[T - 1].err.empty()) {   // trailing bytes the segment walker did not reach
      if (attempt || T == 1) { err = "OTLP protobuf: malformed TracesData"; return false; }
      exact = false;
    }
    if (exact) break;
    if (attempt) { err = "OTLP protobuf: malformed TracesData"; return false; }
  }
  return true;
}

// The TracesData chain alone (the ResourceSpans records).
bool walk_chain(const uint8_t* p, size_t n, std::vector<uint64_t>& res_ref, std::string& err) {
  static const ColumnizeCtx no_ctx;
  static ResCache no_cache;
  std::vector<WalkChunk> ch;
  if (!walk_split(no_ctx, no_cache, p, n, true, true, ch, err)) return false;
  size_t total = 0;
  for (auto& c : ch) total += c.lay.res_ref.size();
  res_ref.resize(total);
  size_t o = 0;
  for (auto& c : ch) {
    std::memcpy(res_ref.data() + o, c.lay.res_ref.data(), 8 * c.lay.res_ref.size());
    o += c.lay.res_ref.size();
  }
  return true;
}

// The whole walk: walk_split's chunks merged.
bool walk(const ColumnizeCtx& ctx, ResCache& cache, const uint8_t* p, size_t n, Walked& w, bool gpu_scopes = false) {
  std::vector<WalkChunk> ch;
  if (!walk_split(ctx, cache, p, n, gpu_scopes, false, ch, w.err)) return false;
  // merge: global indices, attribute sets in first-appearance order
  std::unordered_map<uint32_t, uint32_t> set_map;   // cache id -> this batch's
  {
    std::shared_lock<std::shared_mutex> g(cache.mu);
    for (auto& c : ch)
      for (uint32_t id : c.res_set)
        if (set_map.emplace(id, (uint32_t)w.sets.size()).second) w.sets.push_back(cache.sets[id]);
  }
  size_t nspan = 0, nres = 0, nscope = 0;
  for (size_t t = 0; t < ch.size(); t++) {
    nspan += ch[t].span_ref.size();
    nres += ch[t].res_svc.size();
    nscope += ch[t].scope_size.size();
  }
  w.span_ref.resize(nspan);
  if (!gpu_scopes) {
    w.span_res.resize(nspan);
    w.span_scope.resize(nspan);
  }
  w.scope_on_host.resize(nscope);
  w.scope_count.resize(nscope);
  w.res_svc.resize(nres);
  w.res_svc_str.resize(nres);
  w.res_attrset.resize(nres);
  w.res_size.resize(nres);
  w.res_ok.resize(nres);
  w.res_sql_ok.resize(nres);
  w.attr_res.resize(nres);
  w.scope_size.resize(nscope);
  w.scope_res.resize(nscope);
  w.lay.res_ref.resize(nres);
  w.lay.res_scope0.resize(nres);
  w.lay.scope_ref.resize(nscope);
  w.lay.scope_hdr.resize(nscope);
  w.lay.scope_schema.resize(nscope);
  w.lay.scope_span0.resize(nscope);
  std::vector<size_t> so(ch.size()), ro(ch.size()), co(ch.size());
  for (size_t t = 1; t < ch.size(); t++) {
    so[t] = so[t - 1] + ch[t - 1].span_ref.size();
    ro[t] = ro[t - 1] + ch[t - 1].res_svc.size();
    co[t] = co[t - 1] + ch[t - 1].scope_size.size();
  }
  auto place = [&](size_t t) {
    const WalkChunk& c = ch[t];
    for (size_t k = 0; k < c.span_ref.size(); k++) {
      w.span_ref[so[t] + k] = c.span_ref[k];
      if (!gpu_scopes) {
        w.span_res[so[t] + k] = (uint32_t)(ro[t] + c.span_res[k]);
        w.span_scope[so[t] + k] = (uint32_t)(co[t] + c.span_scope[k]);
      }
    }
    for (size_t k = 0; k < c.res_svc.size(); k++) {
      w.res_svc[ro[t] + k] = c.res_svc[k];
      w.res_svc_str[ro[t] + k] = c.res_svc_str[k];
      w.res_attrset[ro[t] + k] = set_map.at(c.res_set[k]);
      w.res_size[ro[t] + k] = c.res_size[k];
      w.res_ok[ro[t] + k] = c.res_ok[k];
      w.res_sql_ok[ro[t] + k] = c.res_sql_ok[k];
      w.attr_res[ro[t] + k] = c.attr_res[k];
      w.lay.res_ref[ro[t] + k] = c.lay.res_ref[k];
      w.lay.res_scope0[ro[t] + k] = (uint32_t)(co[t] + c.lay.res_scope0[k]);
    }
    for (size_t k = 0; k < c.scope_size.size(); k++) {
      w.scope_size[co[t] + k] = c.scope_size[k];
      w.scope_res[co[t] + k] = (uint32_t)(ro[t] + c.scope_res[k]);
      w.lay.scope_ref[co[t] + k] = c.lay.scope_ref[k];
      w.lay.scope_hdr[co[t] + k] = c.lay.scope_hdr[k];
      w.lay.scope_schema[co[t] + k] = c.lay.scope_schema[k];
      w.lay.scope_span0[co[t] + k] = (uint32_t)(so[t] + c.lay.scope_span0[k]);   // gpu_scopes: into span_ref
      w.scope_on_host[co[t] + k] = c.scope_on_host[k];
      w.scope_count[co[t] + k] = c.scope_count[k];
    }
  };
  parallel_run((int)ch.size(), [&](int t) { place((size_t)t); });
  return true;
}
}  // namespace

// the walk and the spans' sizes for the encoder's CPU test seams (otlp_batch.hpp)
int otlp_host_walk_sizes(const uint8_t* pb, size_t len, std::vector<uint64_t>& span_ref, OtlpLayout& lay,
                         std::vector<uint32_t>& span_size) {
  ColumnizeCtx ctx;
  std::string err = ctx.build(nullptr, nullptr, nullptr);
  Walked w;
  ResCache cache;
  if (err.empty() && !walk(ctx, cache, pb, len, w)) err = w.err;
  if (!err.empty()) return fail(OSE_EINVAL, err);
  span_size.resize(w.span_ref.size());
  ProtoSizer sizer;
  for (size_t i = 0; i < span_size.size(); i++) {
    Span sp;
    if (!pb_span(pb + (uint32_t)w.span_ref[i], (size_t)(w.span_ref[i] >> 32), sp))
      return fail(OSE_EINVAL, "OTLP protobuf: malformed Span");
    span_size[i] = (uint32_t)sizer.span(sp);
  }
  span_ref = std::move(w.span_ref);
  lay = std::move(w.lay);
  return 0;
}

namespace {
// A look-back scan of n counts (launch_scan_u32; none when n is 0).  `status`
// and `words` are zeroed by the caller, which names the words the scan's total,
// tile counter and error go to and reads them back by those indices.
int scan_counts(uint64_t n, uint32_t tiles, const uint32_t* in, uint32_t* out, uint64_t* status, uint32_t* words,
                int total, int counter, int error, hipStream_t st) {
  // (n, n_tiles, popcount, gate, in, out, total, counter, status, error)
  const ScanArgs sa{n, tiles, 0, nullptr, in, out, words + total, words + counter, status, words + error};
  if (n) launch_scan_u32(sa, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The GPU half of the ResourceSpans level: the host walks
// the TracesData chain only (walk_chain), the device each record's fields
// (otlp_res_fields_kernel), the Resource columns from the device resource
// table; resources the table lacks are resolved on the host (pb_resource,
// columnize_resource: the same cache as the host walk), entered into the
// table, and their columns scattered in.  The attribute-set ids are then
// renumbered for the batch (ascending cache id).  *redo: a malformed record
// (the host walk reports it exactly).  Fills w.lay.res_ref and w.sets, *R,
// *S and the args of the scope listing.
// msg_in_stage: the message's H2D copy reads b->stage (a pageable caller
// buffer went through it), so the stage is reused only after that copy
int res_walk_gpu(OtlpEngine* o, OtlpBatchImpl* b, const uint8_t* pb, size_t len, hipStream_t st, Walked& w,
                 uint64_t* R_out, uint64_t* S_out, OtlpResArgs* args, bool* redo, bool msg_in_stage, bool sql) {
  *redo = false;
  std::string err;
  int rc;
  // the TracesData chain: the host walk (it runs while the message's H2D
  // copy is in flight), or (engine option otlp_gpu_chain) segments walked on the GPU
  // and linked here, the host walk when the link fails.  The GPU form
  // measured slower (profiles/r3_otlp_gpu_resources.json host chain,
  // r3_otlp_gpu_chain_gpu_encode.json GPU chain: 10M spans 57.8 -> 97.4 ms of
  // walk, an 8192-span request 0.56 -> 2.06 ms of decode): it cannot
  // start before the whole message has landed, and each lane's hops through
  // its 64 KiB segment are dependent HBM reads.
  std::vector<uint64_t> seg_first;
  std::vector<uint32_t> seg_base;
  uint64_t R = 0;
  bool gpu_chain = len > 0 && b->e->option(Engine::kOptOtlpGpuChain);
  const uint32_t T = (uint32_t)((len + kChainSeg - 1) / kChainSeg);
  OtlpChainArgs ca{};
  if (gpu_chain) {
    const size_t o_end = up(8 * (size_t)T + 16), o_nrec = o_end + up(8 * (size_t)T + 16),
                 o_bad = o_nrec + up(4 * (size_t)T + 16), o_list = o_bad + up(4 * (size_t)T + 16),
                 o_first = o_list + up(8 * (size_t)T * kChainList + 16), o_base = o_first + up(8 * (size_t)T + 16),
                 o_total = o_base + up(4 * (size_t)T + 16);
    if ((rc = b->cslab.need(o_total)) || (rc = b->stage.need(o_first))) return rc;
    HIP_TRY(hipStreamSynchronize(st));   // the staging buffer (the message's H2D) is reused below
    ca.pb = b->arena.p;
    ca.n = len;
    ca.n_seg = T;
    ca.start = reinterpret_cast<uint64_t*>(b->cslab.p);
    ca.end = reinterpret_cast<uint64_t*>(b->cslab.p + o_end);
    ca.nrec = reinterpret_cast<uint32_t*>(b->cslab.p + o_nrec);
    ca.bad = reinterpret_cast<uint32_t*>(b->cslab.p + o_bad);
    ca.list = reinterpret_cast<uint64_t*>(b->cslab.p + o_list);
    ca.first = reinterpret_cast<const uint64_t*>(b->cslab.p + o_first);
    ca.base = reinterpret_cast<const uint32_t*>(b->cslab.p + o_base);
    (void)hipGetLastError();
    launch_otlp_chain_seg(ca, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->stage.p, b->cslab.p, o_first, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t* h_start = reinterpret_cast<const uint64_t*>(b->stage.p);
    const uint64_t* h_end = reinterpret_cast<const uint64_t*>(b->stage.p + o_end);
    const uint32_t* h_nrec = reinterpret_cast<const uint32_t*>(b->stage.p + o_nrec);
    const uint32_t* h_bad = reinterpret_cast<const uint32_t*>(b->stage.p + o_bad);
    const uint64_t* h_list = reinterpret_cast<const uint64_t*>(b->stage.p + o_list);
    // link: the true chain enters segment t at pos; the segment's walk must
    // have a field start there (its speculated start, or where a start
    // inside a record converged), and counts from it
    seg_first.assign(T, kChainNone);
    seg_base.assign(T, 0);
    uint64_t pos = 0;
    for (uint32_t t = 0; t < T && gpu_chain; t++) {
      const uint64_t s1 = std::min<uint64_t>(len, (uint64_t)t * kChainSeg + kChainSeg);
      if (pos >= s1) continue;   // a record covers the whole segment
      if (h_start[t] == kChainNone) { gpu_chain = false; break; }
      uint32_t j = 0, skipped = 0;
      while (j < kChainList && h_list[(uint64_t)t * kChainList + j] != kChainNone &&
             (h_list[(uint64_t)t * kChainList + j] & ~(1ull << 63)) != pos) {
        skipped += (uint32_t)(h_list[(uint64_t)t * kChainList + j] >> 63);
        j++;
      }
      if (j == kChainList || h_list[(uint64_t)t * kChainList + j] == kChainNone || h_bad[t]) { gpu_chain = false; break; }
      seg_first[t] = pos;
      seg_base[t] = (uint32_t)R;
      R += h_nrec[t] - skipped;
      pos = h_end[t];
    }
    if (pos != len) gpu_chain = false;   // the host walk decides (and reports a malformed message)
    if (R > 0xFFFFFFF0ull) gpu_chain = false;
  }
  if (!gpu_chain) {
    if (!walk_chain(pb, len, w.lay.res_ref, err)) return fail(OSE_EINVAL, err);
    // the staging buffer is reused below: wait for the message's H2D when it
    // came through it (a pinned caller buffer is copied from directly, and
    // the resource pass queues behind that copy on the stream)
    if (msg_in_stage) HIP_TRY(hipStreamSynchronize(st));
    R = w.lay.res_ref.size();
  }
  *R_out = R;
  b->walk_info[0] = gpu_chain ? 1u : 0u;
  const uint64_t RN = std::max<uint64_t>(R, 1);
  const uint32_t tiles = (uint32_t)((RN + kScanTileItems - 1) / kScanTileItems);
  OtlpResArgs a{};
  uint64_t* status = nullptr;
  uint32_t* words = nullptr;
  const std::vector<SlabPart> parts = {
      {(void**)&a.res_ref, 8 * RN}, {(void**)&a.flags, 4 * RN}, {(void**)&a.nscope, 4 * RN},
      {(void**)&a.schema_len, 4 * RN}, {(void**)&a.scope0, 4 * RN}, {(void**)&a.res_svc, 4 * RN},
      {(void**)&a.res_svc_str, 4 * RN}, {(void**)&a.res_set, 4 * RN}, {(void**)&a.res_size, 4 * RN},
      {(void**)&a.res_ok, RN}, {(void**)&a.res_sql_ok, sql ? RN : 0}, {(void**)&a.attr_res, 8 * RN},
      {(void**)&a.miss_list, 4 * RN},
      {(void**)&status, 8 * (size_t)tiles + 64}, {(void**)&words, 64},
  };
  if ((rc = slab_place(b->rslab, parts)) || (rc = b->stage.need(std::max<size_t>(8 * RN, 12 * (size_t)T) + 64))) return rc;
  if (!sql) a.res_sql_ok = nullptr;
  if (gpu_chain) {   // the records of the linked segments, written on the GPU
    std::memcpy(b->stage.p, seg_first.data(), 8 * (size_t)T);
    std::memcpy(b->stage.p + 8 * (size_t)T, seg_base.data(), 4 * (size_t)T);
    HIP_TRY(hipMemcpyAsync(const_cast<uint64_t*>(ca.first), b->stage.p, 8 * (size_t)T, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(const_cast<uint32_t*>(ca.base), b->stage.p + 8 * (size_t)T, 4 * (size_t)T,
                           hipMemcpyHostToDevice, st));
    ca.res_ref = const_cast<uint64_t*>(a.res_ref);
    launch_otlp_chain_list(ca, st);
    HIP_TRY(hipGetLastError());
  } else if (R) {
    std::memcpy(b->stage.p, w.lay.res_ref.data(), 8 * R);
    HIP_TRY(hipMemcpyAsync(const_cast<uint64_t*>(a.res_ref), b->stage.p, 8 * R, hipMemcpyHostToDevice, st));
  }
  b->d_res_ref = const_cast<uint64_t*>(a.res_ref);
  HIP_TRY(hipMemsetAsync(status, 0, reinterpret_cast<uint8_t*>(words) + 64 - reinterpret_cast<uint8_t*>(status), st));
  a.pb = b->arena.p;
  a.n_res = R;
  a.any_bad = words;
  a.miss_count = words + 1;
  uint32_t h[4] = {0, 0, 0, 0};
  {
    DevResTable& t = o->res_dev;
    {
      std::unique_lock<std::shared_mutex> g(t.mu);
      if ((rc = t.ensure())) return rc;
    }
    std::shared_lock<std::shared_mutex> g(t.mu);   // held until the lookups have run
    a.table = t.d_slots;
    a.keys = t.d_keys;
    (void)hipGetLastError();
    launch_otlp_res_fields(a, st);
    HIP_TRY(hipGetLastError());
    if ((rc = scan_counts(R, tiles, a.nscope, const_cast<uint32_t*>(a.scope0), status, words, 2, 3, 4, st))) return rc;
    HIP_TRY(hipMemcpyAsync(h, words, 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (h[0]) { *redo = true; return 0; }
  *S_out = h[2];
  // the resources the table lacks: resolved on the host
  const uint32_t nm = h[1];
  b->walk_info[1] = nm;
  if (nm) {
    if (w.lay.res_ref.size() != R) {   // the refs the GPU chain walk wrote
      w.lay.res_ref.resize(R);
      HIP_TRY(hipMemcpy(w.lay.res_ref.data(), a.res_ref, 8 * R, hipMemcpyDeviceToHost));
    }
    std::vector<uint32_t> miss(nm);
    HIP_TRY(hipMemcpy(miss.data(), a.miss_list, 4 * (size_t)nm, hipMemcpyDeviceToHost));
    std::vector<OtlpResFix> fix(nm);
    std::vector<uint8_t> keyed(nm, 0);   // entered into the device table (one Resource field or none)
    std::vector<std::pair<size_t, size_t>> key_of(nm);
    const int T = (int)std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)parallel_width(), nm / 256));
    std::vector<std::string> errs((size_t)T);
    parallel_run(T, [&](int t) {
      ProtoSizer sizer;
      std::vector<std::pair<size_t, size_t>> resf;
      for (uint32_t k = (uint32_t)((uint64_t)nm * t / T); k < (uint32_t)((uint64_t)nm * (t + 1) / T); k++) {
        const uint32_t r = miss[k];
        const uint64_t rr = w.lay.res_ref[r];
        if (!res_record_fields(pb, (uint32_t)rr, (size_t)(rr >> 32), resf)) {
          errs[t] = "OTLP protobuf: malformed ResourceSpans";
          return;
        }
        CachedRes cr{};
        if (!cached_resource(o->ctx, o->res_cache, pb, resf, sizer, cr)) {
          errs[t] = "OTLP protobuf: malformed Resource";
          return;
        }
        fix[k] = OtlpResFix{r, cr.svc, cr.svc_str, cr.set, cr.rpart, (uint32_t)cr.ok | ((uint32_t)cr.sql_ok << 1), cr.attr_res};
        if (resf.size() <= 1) {
          keyed[k] = 1;
          key_of[k] = resf.empty() ? std::pair<size_t, size_t>(0, 0) : resf[0];
        }
      }
    });
    for (auto& e : errs)
      if (!e.empty()) return fail(OSE_EINVAL, e);
    if ((rc = b->fixdev.need(sizeof(OtlpResFix) * nm)) || (rc = b->stage.need(sizeof(OtlpResFix) * nm))) return rc;
    std::memcpy(b->stage.p, fix.data(), sizeof(OtlpResFix) * nm);
    HIP_TRY(hipMemcpyAsync(b->fixdev.p, b->stage.p, sizeof(OtlpResFix) * nm, hipMemcpyHostToDevice, st));
    launch_otlp_res_fix(a, reinterpret_cast<const OtlpResFix*>(b->fixdev.p), nm, st);
    HIP_TRY(hipGetLastError());
    {   // later calls find these on the device
      DevResTable& t = o->res_dev;
      std::unique_lock<std::shared_mutex> g(t.mu);
      for (uint32_t k = 0; k < nm; k++) {
        if (!keyed[k]) continue;
        const CachedRes cr{fix[k].svc, fix[k].svc_str, fix[k].set, fix[k].rpart, (uint8_t)(fix[k].ok & 1), fix[k].attr_res,
                           (uint8_t)(fix[k].ok >> 1)};
        t.insert(pb + key_of[k].first, (uint32_t)key_of[k].second, cr);
      }
      if ((rc = t.sync(st))) return rc;
    }
    for (uint32_t k = 0; k < nm; k++) b->walk_info[2] += keyed[k];
  }
  // the cache's attribute-set ids -> this batch's (first appearance)
  uint32_t n_sets;
  {
    std::shared_lock<std::shared_mutex> g(o->res_cache.mu);
    n_sets = (uint32_t)o->res_cache.sets.size();
  }
  const uint64_t NS = std::max<uint64_t>(n_sets, 1);
  const size_t o_flag = up(4 * NS + 16), o_pos = o_flag + up(4 * RN + 16), o_list = o_pos + up(4 * RN + 16),
               o_stat = o_list + up(4 * RN + 16), o_words = o_stat + up(8 * (size_t)tiles + 64);
  if ((rc = b->setbuf.need(o_words + 64))) return rc;
  uint32_t* first = reinterpret_cast<uint32_t*>(b->setbuf.p);
  uint32_t* is_first = reinterpret_cast<uint32_t*>(b->setbuf.p + o_flag);
  uint32_t* pos = reinterpret_cast<uint32_t*>(b->setbuf.p + o_pos);
  uint32_t* list = reinterpret_cast<uint32_t*>(b->setbuf.p + o_list);
  uint64_t* sstat = reinterpret_cast<uint64_t*>(b->setbuf.p + o_stat);
  uint32_t* swords = reinterpret_cast<uint32_t*>(b->setbuf.p + o_words);
  HIP_TRY(hipMemsetAsync(first, 0xFF, 4 * NS, st));
  HIP_TRY(hipMemsetAsync(sstat, 0, o_words + 64 - o_stat, st));
  launch_otlp_set_first(a.res_set, R, first, is_first, st);
  HIP_TRY(hipGetLastError());
  if ((rc = scan_counts(R, tiles, is_first, pos, sstat, swords, 1, 2, 0, st))) return rc;
  launch_otlp_set_apply(a.res_set, R, first, is_first, pos, list, st);
  HIP_TRY(hipGetLastError());
  // the scan's words and the batch's set ids come back behind the scope
  // pass, whose wait the host makes anyway (res_sets_finish)
  if ((rc = b->seth.need(4 * (RN + 2)))) return rc;
  uint32_t* hs = reinterpret_cast<uint32_t*>(b->seth.p);
  HIP_TRY(hipMemcpyAsync(hs, swords, 8, hipMemcpyDeviceToHost, st));
  if (R) HIP_TRY(hipMemcpyAsync(hs + 2, list, 4 * R, hipMemcpyDeviceToHost, st));
  *args = a;
  b->d_res_scope0 = const_cast<uint32_t*>(a.scope0);
  b->d_attr_res = a.attr_res;
  return 0;
}

// the batch's attribute sets from res_walk_gpu's copies (first appearance)
int res_sets_finish(OtlpEngine* o, OtlpBatchImpl* b, Walked& w, hipStream_t st) {
  HIP_TRY(hipStreamSynchronize(st));   // (the scope pass has waited already: returns at once)
  const uint32_t* hs = reinterpret_cast<const uint32_t*>(b->seth.p);
  if (hs[0]) return fail(OSE_EDEVICE, "OTLP ingest: attribute-set scan error");
  std::shared_lock<std::shared_mutex> g(o->res_cache.mu);
  w.sets.clear();
  for (uint32_t k = 0; k < hs[1]; k++) w.sets.push_back(o->res_cache.sets[hs[2 + k]]);
  return 0;
}

// The GPU half of the structural walk: every ScopeSpans the host did not
// walk is counted, sized and listed on the device (otlp_scope_*_kernel);
// returns the span count in *n_out, or 1 in *redo when some scope needs the
// host walk (groups or a malformed field: the caller walks on the host).
// res: the GPU ResourceSpans pass ran (res_walk_gpu): its S scopes are listed
// on the device by otlp_res_scopes_kernel, every one walked here
int scope_walk_gpu(Engine* e, OtlpBatchImpl* b, Walked& w, hipStream_t st, uint64_t* n_out, bool* redo,
                   OtlpResArgs* res = nullptr, uint64_t S_res = 0) {
  (void)e;
  const uint64_t S = res ? S_res : w.scope_size.size(), H = res ? 0 : w.span_ref.size();
  *redo = false;
  const uint32_t tiles = (uint32_t)((S + kScanTileItems - 1) / kScanTileItems);
  uint64_t *scope_ref, *hdr, *schema, *host_at, *host_refs, *status;
  uint8_t* on_host;
  uint32_t *count, *scope_size, *flags, *span0, *scope_res, *words;
  const std::vector<SlabPart> parts = {
      {(void**)&scope_ref, 8 * S, res ? nullptr : b->lay.scope_ref.data()},
      {(void**)&hdr, 8 * S, res ? nullptr : b->lay.scope_hdr.data()},
      {(void**)&schema, 8 * S, res ? nullptr : b->lay.scope_schema.data()},
      {(void**)&host_at, 8 * S, nullptr, !res},   // filled in staging below
      {(void**)&host_refs, 8 * H, res ? nullptr : w.span_ref.data()},
      {(void**)&on_host, S, res ? nullptr : w.scope_on_host.data()},
      {(void**)&count, 4 * S, res ? nullptr : w.scope_count.data()},
      {(void**)&scope_size, 4 * S, res ? nullptr : w.scope_size.data()},
      {(void**)&scope_res, 4 * S, res ? nullptr : w.scope_res.data()},
      // device-only
      {(void**)&flags, 4 * S},
      {(void**)&span0, 4 * S},
      {(void**)&status, 8 * (size_t)tiles + 64},
      {(void**)&words, 64},
  };
  SlabSize z;
  int rc;
  if ((rc = slab_place(b->sslab, parts, &b->stage, &z))) return rc;
  if (!res) {   // host_at: the host-walked scopes' offsets into host_refs (the walk's span0)
    uint64_t* ha = reinterpret_cast<uint64_t*>(b->stage.p + (reinterpret_cast<uint8_t*>(host_at) - b->sslab.p));
    for (uint64_t q = 0; q < S; q++) ha[q] = b->lay.scope_span0[q];
    HIP_TRY(hipMemcpyAsync(b->sslab.p, b->stage.p, z.inputs, hipMemcpyHostToDevice, st));
  } else {
    // the scopes of every resource at their place, none walked on the host
    HIP_TRY(hipMemsetAsync(on_host, 0, S, st));
    res->scope_ref = scope_ref;
    res->scope_res = scope_res;
    launch_otlp_res_scopes(*res, st);
    HIP_TRY(hipGetLastError());
    b->d_scope_ref = scope_ref;
  }
  const size_t dev0 = reinterpret_cast<uint8_t*>(flags) - b->sslab.p;
  HIP_TRY(hipMemsetAsync(flags, 0, z.total - dev0, st));   // flags, span0, scan status, words
  OtlpScopeArgs a{};
  a.pb = b->arena.p;
  a.n_scopes = S;
  a.scope_ref = scope_ref;
  a.on_host = on_host;
  a.scope_res = scope_res;
  a.count = count;
  a.scope_size = scope_size;
  a.hdr = hdr;
  a.schema = schema;
  a.flags = flags;
  a.span0 = span0;
  a.host_refs = host_refs;
  a.host_at = host_at;
  b->sargs = a;
  (void)hipGetLastError();
  launch_otlp_scope_count(a, st);
  HIP_TRY(hipGetLastError());
  if ((rc = scan_counts(S, tiles, count, span0, status, words, 1, 2, 0, st))) return rc;
  uint32_t h[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(h, words, 8, hipMemcpyDeviceToHost, st));
  // which scopes the host must finish (flags): copied back with the counts
  std::vector<uint32_t> fl(S);
  if (S) HIP_TRY(hipMemcpyAsync(fl.data(), flags, 4 * S, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h[0]) return fail(OSE_EDEVICE, "OTLP ingest: scope scan error");
  *n_out = h[1];
  b->d_span0 = span0;
  b->d_hdr = hdr;
  b->d_schema = schema;
  std::vector<std::pair<uint64_t, uint32_t>> patch;   // scope sizes the host computes
  ProtoSizer sizer;
  if (res) {
    bool any = false;
    for (uint64_t q = 0; q < S && !any; q++) any = fl[q] != 0;
    if (any) {   // the flagged scopes' refs
      b->lay.scope_ref.resize(S);
      HIP_TRY(hipMemcpy(b->lay.scope_ref.data(), scope_ref, 8 * S, hipMemcpyDeviceToHost));
    }
  }
  for (uint64_t q = 0; q < S; q++) {
    if (!fl[q]) continue;
    if (fl[q] & 2) { *redo = true; return 0; }
    // a merged or unusual InstrumentationScope: pb_scope over its fields
    const uint64_t sr = b->lay.scope_ref[q];
    PbReader r(b->pb + (uint32_t)sr, (size_t)(sr >> 32));
    ScopeSpans meta;
    size_t sch = 0;
    uint32_t f, wt;
    while (r.more() && r.tag(f, wt)) {
      size_t o, l;
      if ((f == 1 || f == 2 || f == 3) && wt == 2 && r.bytes(o, l)) {
        if (f == 1 && !pb_scope(b->pb + (uint32_t)sr + o, l, meta))
          return fail(OSE_EINVAL, "OTLP protobuf: malformed InstrumentationScope");
        if (f == 3) sch = l;
      } else if (f == 1 || f == 2 || f == 3) {
        return fail(OSE_EINVAL, "OTLP protobuf: malformed ScopeSpans");
      } else {
        r.skip(wt, f);
      }
    }
    if (!r.ok) return fail(OSE_EINVAL, "OTLP protobuf: malformed ScopeSpans");
    patch.emplace_back(q, (uint32_t)(sizer.scope_fixed(meta) + (sch ? flen(sch) : 0)));
  }
  b->walk_info[3] = (uint32_t)patch.size();
  for (auto& x : patch) HIP_TRY(hipMemcpyAsync(scope_size + x.first, &x.second, 4, hipMemcpyHostToDevice, st));
  if (!patch.empty()) HIP_TRY(hipStreamSynchronize(st));   // the patch sources are on this stack
  b->cols.scope_size = scope_size;
  b->cols.scope_resource = scope_res;
  // pass 2 writes into the span columns decode() allocates next
  b->layout_on_host = false;
  return 0;
}
}  // namespace

// span refs and the scopes' span0 / header / schema refs back to the host
// (the encoder and the host pass read them there)
int layout_to_host(OtlpBatchImpl* b, hipStream_t st) {
  if (b->layout_on_host) return 0;
  const uint64_t n = b->cols.n_spans, S = b->cols.n_scopes, R = b->cols.n_resources;
  b->span_ref.resize(n);
  std::vector<uint32_t> span0(S);
  if (b->res_on_device) {   // the ResourceSpans level was walked on the GPU too
    if (b->lay.res_ref.size() != R) {
      b->lay.res_ref.resize(R);
      if (R) HIP_TRY(hipMemcpyAsync(b->lay.res_ref.data(), b->d_res_ref, 8 * R, hipMemcpyDeviceToHost, st));
    }
    b->lay.res_scope0.resize(R);
    b->lay.scope_ref.resize(S);
    b->lay.scope_hdr.resize(S);
    b->lay.scope_schema.resize(S);
    b->lay.scope_span0.resize(S);
    if (R) HIP_TRY(hipMemcpyAsync(b->lay.res_scope0.data(), b->d_res_scope0, 4 * R, hipMemcpyDeviceToHost, st));
    if (S) HIP_TRY(hipMemcpyAsync(b->lay.scope_ref.data(), b->d_scope_ref, 8 * S, hipMemcpyDeviceToHost, st));
  }
  if (n) HIP_TRY(hipMemcpyAsync(b->span_ref.data(), b->d_span_ref, 8 * n, hipMemcpyDeviceToHost, st));
  if (S) {
    HIP_TRY(hipMemcpyAsync(span0.data(), b->d_span0, 4 * S, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b->lay.scope_hdr.data(), b->d_hdr, 8 * S, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b->lay.scope_schema.data(), b->d_schema, 8 * S, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  for (uint64_t q = 0; q < S; q++) b->lay.scope_span0[q] = span0[q];
  b->layout_on_host = true;
  return 0;
}

// (walk_info[7] says that the arena was regrown)
int regrow_arena(OtlpBatchImpl* b, size_t keep, size_t want, hipStream_t st) {
  if (want <= b->arena.cap) return 0;
  DevBuf bigger;
  if (int rc = bigger.need(want)) return rc;
  HIP_TRY(hipMemcpyAsync(bigger.p, b->arena.p, keep, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));   // the old arena is freed on return
  std::swap(b->arena.p, bigger.p);
  std::swap(b->arena.cap, bigger.cap);
  b->cols.arena = b->arena.p;
  b->walk_info[7] = 1;
  return 0;
}

namespace {
// ---- ose_otlp_decode's steps (decode() below calls them in this order) ----------
// Engine option otlp_url_full: the per-span decoded lengths, their exclusive
// scan and the scan's tile status (column_slab carves them), and the words
// that follow the host list's count under the option, fetched with it
struct UrlFullCols { uint32_t *dec_len = nullptr, *dec_off = nullptr; uint64_t* status = nullptr; uint32_t tiles = 0; };
enum : int { kUfTotal = 1, kUfParsed = 2, kUfScanError = 3, kUfCounter = 4 };   // [0]: the list's count
constexpr size_t kUfWordBytes = 32;
// the span columns as the span kernel and the host pass's fix kernel write them
template <class Args>
void set_span_columns(Args& a, const ose_columns& c) {
  a.tid = const_cast<uint64_t*>(c.trace_id);
  a.start = const_cast<uint64_t*>(c.start_ns);
  a.end = const_cast<uint64_t*>(c.end_ns);
  a.status = const_cast<uint8_t*>(c.status);
  a.kind = const_cast<uint8_t*>(c.kind);
  a.url_flags = const_cast<uint8_t*>(c.url_flags);
  a.path = const_cast<ose_strref*>(c.path);
  a.route = const_cast<ose_strref*>(c.route);
  a.span_size = const_cast<uint32_t*>(c.span_size);
  a.name_len = const_cast<uint32_t*>(c.name_len);
  a.attr_match = const_cast<uint64_t*>(c.attr_match);
  a.attr_type = const_cast<uint8_t*>(c.attr_type);
  a.attr_val = const_cast<uint64_t*>(c.attr_val);
}

// 1. the bytes H2D into the arena, zero slack behind them: straight from the
//    caller's buffer when it is pinned (*pinned), else through pinned staging
int upload_message(OtlpBatchImpl* b, const uint8_t* pb, size_t len, hipStream_t st, bool* pinned) {
  int rc;
  const size_t pb_cap = up(len + 16, 16);
  const size_t fix_reserve = std::max<size_t>(1 << 16, len / 8);
  if ((rc = b->arena.need(pb_cap + fix_reserve + 16))) return rc;
  hipPointerAttribute_t pa{};
  *pinned = len && hipPointerGetAttributes(&pa, pb) == hipSuccess && pa.type == hipMemoryTypeHost;
  (void)hipGetLastError();   // an unregistered pointer is not an error here
  if (*pinned) {
    HIP_TRY(hipMemcpyAsync(b->arena.p, pb, len, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(b->arena.p + len, 0, pb_cap - len, st));
  } else {
    if ((rc = b->stage.need(pb_cap))) return rc;
    par_memcpy(b->stage.p, pb, len);
    std::memset(b->stage.p + len, 0, pb_cap - len);
    HIP_TRY(hipMemcpyAsync(b->arena.p, b->stage.p, pb_cap, hipMemcpyHostToDevice, st));
  }
  return 0;
}

// 2a. the walk: ResourceSpans on the GPU behind the host's chain walk (gpu_res:
//     *ra, *R, *S filled; *redo: a malformed record), else the host walk
int walk_records(OtlpEngine* o, OtlpBatchImpl* b, const uint8_t* pb, size_t len, hipStream_t st, bool gpu_scopes,
                 bool gpu_res, bool msg_in_stage, bool sql, Walked& w, OtlpResArgs* ra, uint64_t* R, uint64_t* S,
                 bool* redo) {
  if (gpu_res) return res_walk_gpu(o, b, pb, len, st, w, R, S, ra, redo, msg_in_stage, sql);
  if (!walk(o->ctx, o->res_cache, pb, len, w, gpu_scopes)) return fail(OSE_EINVAL, w.err);
  HIP_TRY(hipStreamSynchronize(st));   // the staging buffer is reused below
  *R = w.res_svc.size();
  return 0;
}

// 2b. the batch takes the walk's layout; the ScopeSpans the host left are walked
//     on the GPU (*redo: one needs the host walk).  *n: the spans, *S: the scopes.
int walk_scopes(Engine* e, OtlpEngine* o, OtlpBatchImpl* b, const uint8_t* pb, size_t len, hipStream_t st,
                bool gpu_scopes, bool gpu_res, Walked& w, OtlpResArgs* ra, uint64_t R, uint64_t* S, uint64_t* n,
                bool* redo) {
  b->pb = pb;
  b->pb_len = len;
  b->lay = std::move(w.lay);
  b->layout_on_host = true;
  b->res_on_device = gpu_res;
  b->cols = ose_columns{};
  b->cols.n_resources = (uint32_t)R;
  b->scopes_dev = false;
  if (gpu_scopes) {
    int rc = scope_walk_gpu(e, b, w, st, n, redo, gpu_res ? ra : nullptr, *S);
    if (gpu_res) {   // (also before an error return or a redo: no copy into seth may stay in flight)
      const int src = res_sets_finish(o, b, w, st);
      if (!rc) rc = src;
    }
    if (rc || *redo) return rc;
    b->scopes_dev = true;
  } else {
    *n = w.span_ref.size();
    b->span_ref = std::move(w.span_ref);
  }
  if (!gpu_res) *S = b->lay.scope_ref.size();
  if (*n > 0xFFFFFFF0ull) return fail(OSE_ERANGE, "OTLP ingest: more than 2^32-16 spans");
  return 0;
}

// 2c. the device columns, one slab: the walk's arrays that the GPU walks did
//     not leave on the device go up through staging, the span kernels' outputs
//     follow.  *span_ref_out: the spans' refs, *hl: the host-pass list (count zeroed).
int column_slab(OtlpEngine* o, OtlpBatchImpl* b, Walked& w, const OtlpResArgs& ra, bool gpu_scopes, bool gpu_res,
                bool sql, uint64_t n, uint64_t R, uint64_t S, hipStream_t st, uint64_t** span_ref_out, HostList* hl,
                UrlFullCols* uf) {
  ose_columns& c = b->cols;   // (scope_size / scope_resource are set by the GPU scope walk)
  const uint32_t K = o->n_attr_keys;
  b->attrsets = std::move(w.sets);
  const uint64_t N = std::max<uint64_t>(n, 1);
  uint64_t*& span_ref = *span_ref_out;
  hl->cap = (uint32_t)N;
  std::vector<SlabPart> parts = {
      {(void**)&span_ref, 8 * N, gpu_scopes ? nullptr : b->span_ref.data()},
      {(void**)&c.resource, 4 * N, gpu_scopes ? nullptr : w.span_res.data()},
      {(void**)&c.scope, 4 * N, gpu_scopes ? nullptr : w.span_scope.data()},
  };
  if (!gpu_res) {
    parts.push_back({(void**)&c.res_svc, 4 * R, w.res_svc.data()});
    parts.push_back({(void**)&c.res_svc_str, 4 * R, w.res_svc_str.data()});
    parts.push_back({(void**)&c.res_url_ok, R, w.res_ok.data()});
    parts.push_back({(void**)&c.res_attrset, 4 * R, w.res_attrset.data()});
    parts.push_back({(void**)&c.res_size, 4 * R, w.res_size.data()});
    if (sql) parts.push_back({(void**)&c.res_sql_ok, R, w.res_sql_ok.data()});
  }
  if (!gpu_scopes) {
    parts.push_back({(void**)&c.scope_size, 4 * S, w.scope_size.data()});
    parts.push_back({(void**)&c.scope_resource, 4 * S, w.scope_res.data()});
  }
  parts.insert(parts.end(), {
      // outputs of the decoder
      {(void**)&c.trace_id, 16 * N}, {(void**)&c.start_ns, 8 * N}, {(void**)&c.end_ns, 8 * N},
      {(void**)&c.status, N}, {(void**)&c.kind, N}, {(void**)&c.url_flags, N},
      {(void**)&c.path, 8 * N}, {(void**)&c.route, 8 * N}, {(void**)&c.span_size, 4 * N},
      {(void**)&c.name_len, 4 * N},
      {(void**)&hl->flag, N}, {(void**)&hl->count, uf ? kUfWordBytes : 16}, {(void**)&hl->list, 4 * N},
  });
  if (uf) {   // engine option otlp_url_full: the decoded lengths, their scan and its tile status
    uf->tiles = (uint32_t)((N + kScanTileItems - 1) / kScanTileItems);
    parts.push_back({(void**)&uf->dec_len, 4 * N});
    parts.push_back({(void**)&uf->dec_off, 4 * N});
    parts.push_back({(void**)&uf->status, 8 * (size_t)uf->tiles});
  }
  if (o->json_rules) parts.push_back({(void**)&c.attr_match, 8 * N * (size_t)o->attr_words});
  if (sql) {
    parts.push_back({(void**)&c.db_flags, N});
    parts.push_back({(void**)&c.db_query, 8 * N});
  }
  if (K) {
    parts.push_back({(void**)&c.attr_type, (size_t)K * N});
    parts.push_back({(void**)&c.attr_val, 8 * (size_t)K * N});
  }
  SlabSize z;
  if (int rc = slab_place(b->slab, parts, &b->stage, &z)) return rc;
  if (z.inputs) HIP_TRY(hipMemcpyAsync(b->slab.p, b->stage.p, z.inputs, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(hl->count, 0, uf ? kUfWordBytes : 16, st));
  if (uf) HIP_TRY(hipMemsetAsync(uf->status, 0, 8 * (size_t)uf->tiles, st));
  if (gpu_res) {   // the resource columns the GPU pass wrote
    c.res_svc = ra.res_svc;
    c.res_svc_str = ra.res_svc_str;
    c.res_url_ok = ra.res_ok;
    c.res_attrset = ra.res_set;
    c.res_size = ra.res_size;
    c.res_sql_ok = ra.res_sql_ok;
  }
  if (gpu_scopes) {
    // pass 2: the span refs of every scope at their place
    OtlpScopeArgs sa = b->sargs;
    sa.span_ref = span_ref;
    sa.span_res = const_cast<uint32_t*>(c.resource);
    sa.span_scope = const_cast<uint32_t*>(c.scope);
    launch_otlp_scope_spans(sa, st);
    HIP_TRY(hipGetLastError());
    b->d_span_ref = span_ref;
    b->d_span_res = const_cast<uint32_t*>(c.resource);
    b->span_ref.clear();
  }
  b->d_spans = span_ref;
  c.n_spans = n;
  c.n_scopes = (uint32_t)S;   // (n_resources: walk_scopes)
  c.n_attrsets = (uint32_t)b->attrsets.size();
  c.arena = b->arena.p;
  c.arena_bytes = b->pb_len;
  c.n_attr_keys = K;
  c.attr_match_words = o->attr_words;
  if (!o->ctx.url_filter) c.res_url_ok = nullptr;
  return 0;
}

// 3. the GPU decoder: otlp_span_kernel, then (sql) otlp_sqlop_kernel and (ca)
//    otlp_condattr_kernel; *cnt: the spans on the host-pass list once they have run
int span_kernels(Engine* e, OtlpEngine* o, OtlpBatchImpl* b, uint64_t n, const uint64_t* span_ref, const HostList& hl,
                 bool sql, bool ca, const UrlFullCols* uf, hipStream_t st, uint32_t* cnt) {
  const ose_columns& c = b->cols;
  OtlpArgs a{};
  a.pb = b->arena.p;
  a.n_spans = n;
  a.span_ref = span_ref;
  a.keys = reinterpret_cast<const OtlpKeyDev*>(o->keys_dev);
  a.key_bytes = o->keys_dev + o->keys.size() * sizeof(OtlpKeyDev);
  a.n_keys = (uint32_t)o->keys.size();
  a.n_attr_keys = o->n_attr_keys;
  a.attr_words = o->attr_words;
  a.key_lens = o->key_lens;
  set_span_columns(a, c);
  set_host_list(a, hl);
  a.url_full = uf ? 1u : 0u;
  (void)hipGetLastError();   // a stale error of an earlier call must not be reported as this launch's
  if (const int rc = e->timed("otlp_span_kernel", st, [&] {
        if (n) b->walk_info[6] = launch_otlp_spans(a, st);
      }))
    return rc;
  if (sql && n) {   // db_flags / db_query: a pass of its own (the span kernels stay within their register budget)
    OtlpSqlArgs qa{};
    qa.pb = b->arena.p;
    qa.n_spans = n;
    qa.span_ref = span_ref;
    qa.db_flags = const_cast<uint8_t*>(c.db_flags);
    qa.db_query = const_cast<ose_strref*>(c.db_query);
    set_host_list(qa, hl);
    if (const int rc = e->timed("otlp_sqlop_kernel", st, [&] { launch_otlp_sqlop(qa, st); })) return rc;
  }
  if (ca)
    if (int rc = condattr_spans(e, b, n, span_ref, hl, st)) return rc;
  if (uf && n) {
    // the Path of url.full / http.url: a pass of its own, last, so the list it
    // skips is final; then the decoded paths' places in span order (the same
    // arena on every run)
    OtlpUrlFullArgs ua{};
    ua.pb = b->arena.p;
    ua.n_spans = n;
    ua.span_ref = span_ref;
    ua.url_flags = const_cast<uint8_t*>(c.url_flags);
    ua.path = const_cast<ose_strref*>(c.path);
    ua.dec_len = uf->dec_len;
    ua.parsed = hl.count + kUfParsed;
    set_host_list(ua, hl);
    if (const int rc = e->timed("otlp_url_full_kernel", st, [&] { launch_otlp_url_full(ua, st); })) return rc;
    if (const int rc = scan_counts(n, uf->tiles, uf->dec_len, uf->dec_off, uf->status, hl.count, kUfTotal, kUfCounter,
                                   kUfScanError, st))
      return rc;
  }
  uint32_t h[4] = {0, 0, 0, 0};   // the list's count; under otlp_url_full the words beside it ride along
  HIP_TRY(hipMemcpyAsync(h, hl.count, uf ? 16 : 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h[kUfScanError]) return fail(OSE_EDEVICE, "OTLP ingest: url.full scan error");
  *cnt = h[0];
  b->host_spans = *cnt;
  b->url_full_counts[0] = h[kUfParsed];
  b->url_full_counts[1] = h[kUfTotal];
  return 0;
}

// 4b. engine option otlp_url_full: the url.full paths that hold escapes,
//     unescaped behind what the arena holds (the message bytes, then the host
//     pass's strings; 16 bytes of slack between and after)
int url_full_unescape(OtlpBatchImpl* b, const UrlFullCols& uf, hipStream_t st) {
  ose_columns& c = b->cols;
  const uint64_t total = b->url_full_counts[1];
  const size_t base = up(c.arena_bytes + 16, 16), end = base + total;
  if (end > 0xFFFFFFF0ull) return fail(OSE_ERANGE, "OTLP ingest: the arena passes 4 GiB");
  if (int rc = regrow_arena(b, base, end + 16, st)) return rc;   // what the arena holds moves with it, slack included
  OtlpUrlFullArgs ua{};
  ua.pb = b->arena.p;
  ua.out = b->arena.p;
  ua.n_spans = c.n_spans;
  ua.url_flags = const_cast<uint8_t*>(c.url_flags);
  ua.path = const_cast<ose_strref*>(c.path);
  ua.dec_len = uf.dec_len;
  ua.dec_off = uf.dec_off;
  ua.dec_base = (uint32_t)base;
  if (const int rc = b->e->timed("otlp_url_full_unescape_kernel", st, [&] { launch_otlp_url_full_unescape(ua, st); }))
    return rc;
  c.arena_bytes = end;
  return 0;
}

// 4. the host pass over the `cnt` listed spans (list: their indices, fetched
//    here): the records and the strings go up through staging
int host_pass(OtlpEngine* o, OtlpBatchImpl* b, const uint8_t* pb, Walked& w, bool gpu_res, bool sql, uint32_t cnt,
              const uint32_t* host_list, hipStream_t st, std::vector<uint32_t>& list) {
  int rc;
  ose_columns& c = b->cols;
  const uint64_t n = c.n_spans, R = c.n_resources;
  const uint32_t K = o->n_attr_keys;
  std::vector<uint64_t>& attr_res = w.attr_res;
  std::vector<uint32_t> span_res;
  const std::vector<uint32_t>* sres = &w.span_res;
  if (gpu_res && !o->wide_host_rules) {   // the resources' span_attribute service bits from the device
    attr_res.resize(R);
    if (R) HIP_TRY(hipMemcpy(attr_res.data(), b->d_attr_res, 8 * R, hipMemcpyDeviceToHost));
  }
  std::vector<uint32_t> res_svc_h;   // wide_host_rules: the resources' service ids
  if (o->wide_host_rules) {
    if (gpu_res) {
      res_svc_h.resize(R);
      if (R) HIP_TRY(hipMemcpy(res_svc_h.data(), c.res_svc, 4 * R, hipMemcpyDeviceToHost));
    } else {
      res_svc_h = w.res_svc;
    }
  }
  if (!b->layout_on_host) {   // the spans' refs and resources from the device
    if ((rc = layout_to_host(b, st))) return rc;
    span_res.resize(n);
    HIP_TRY(hipMemcpy(span_res.data(), b->d_span_res, 4 * n, hipMemcpyDeviceToHost));
    sres = &span_res;
  }
  list.resize(cnt);
  HIP_TRY(hipMemcpy(list.data(), host_list, 4 * (size_t)cnt, hipMemcpyDeviceToHost));
  std::vector<OtlpFix> fix(cnt);
  std::vector<uint8_t> fix_type((size_t)cnt * K);
  std::vector<uint64_t> fix_val((size_t)cnt * K);
  const uint32_t AW = o->json_rules ? o->attr_words : 0;   // attr_match words the host pass writes per span
  std::vector<uint64_t> fix_attr((size_t)cnt * AW);
  std::vector<OtlpSqlFix> fix_sql(sql ? cnt : 0);   // db_flags / db_query (AsString included) of the listed spans
  std::string strs;   // appended after the message bytes and their zero slack
  const size_t str_base = up(b->pb_len + 16, 16);
  auto put = [&](std::string_view s) {
    ose_strref r{(uint32_t)(str_base + strs.size()), (uint32_t)s.size()};
    strs += s;
    return r;
  };
  SpanCols sc;
  ProtoSizer sizer;
  std::vector<uint64_t> res_words;
  for (uint32_t q = 0; q < cnt; q++) {
    const uint32_t i = list[q];
    const uint64_t ref = b->span_ref[i];
    Span sp;
    if (!pb_span(pb + (uint32_t)ref, (size_t)(ref >> 32), sp)) return fail(OSE_EINVAL, "OTLP protobuf: malformed Span");
    if (o->wide_host_rules) {
      const uint32_t sv = res_svc_h[(*sres)[i]];
      if (sv < o->host_rules_by_svc.size()) res_words = o->host_rules_by_svc[sv];
      else res_words.assign(std::max<size_t>(1, o->ctx.attr_plan.host_mask.size()), 0);
    } else {
      host_rule_words(o->ctx.attr_plan, attr_res[(*sres)[i]], res_words);
    }
    columnize_span(o->ctx, sp, res_words, sizer, sc);
    for (uint32_t w = 0; w < AW; w++) fix_attr[(size_t)q * AW + w] = w < sc.attr_match.size() ? sc.attr_match[w] : 0;
    OtlpFix& x = fix[q];
    x = OtlpFix{};
    x.idx = i;
    x.hi = sc.hi;
    x.lo = sc.lo;
    x.start = sc.start;
    x.end = sc.end;
    x.status = sc.status;
    x.kind = sc.kind;
    x.url_flags = sc.url_flags;
    x.span_size = sc.span_size;
    x.name_len = sc.name_len;
    for (uint32_t k = 0; k < K; k++) {
      uint64_t v = sc.attr_val[k];
      if (sc.attr_type[k] == OSE_ATTR_STR) {
        const ose_strref r = put(sc.attr_str[k]);
        v = (uint64_t)r.off | ((uint64_t)r.len << 32);
      }
      fix_type[(size_t)q * K + k] = sc.attr_type[k];
      fix_val[(size_t)q * K + k] = v;
    }
    x.route = sc.has_route ? put(sc.route) : ose_strref{0, 0};
    x.path = (sc.url_flags & OSE_URL_PATH_MASK) != OSE_URL_PATH_NONE ? put(sc.path) : ose_strref{0, 0};
    if (sql)
      fix_sql[q] = OtlpSqlFix{i, sc.db_flags, (sc.db_flags & OSE_DB_HAS_QUERY) ? put(sc.db_query) : ose_strref{0, 0}};
  }
  if ((rc = regrow_arena(b, str_base, str_base + strs.size() + 16, st))) return rc;   // the message bytes move with it
  c.arena_bytes = str_base + strs.size();
  // the records' layout, the same in staging and on the device (plain sums:
  // the OtlpFix part has no 16-byte slack, so the slab carver's rule is not it)
  const size_t fb = up(cnt * sizeof(OtlpFix)), tb = up((size_t)cnt * K + 16), vb = up((size_t)cnt * K * 8 + 16);
  const size_t ab = up((size_t)cnt * AW * 8 + 16), qb = up(fix_sql.size() * sizeof(OtlpSqlFix) + 16);
  const size_t fixb = fb + tb + vb + ab + qb;
  DevBuf& fixdev = b->fixdev;
  if ((rc = b->stage.need(fixb + strs.size() + 16)) || (rc = fixdev.need(fixb))) return rc;
  std::memcpy(b->stage.p, fix.data(), cnt * sizeof(OtlpFix));
  if (K) {
    std::memcpy(b->stage.p + fb, fix_type.data(), (size_t)cnt * K);
    std::memcpy(b->stage.p + fb + tb, fix_val.data(), (size_t)cnt * K * 8);
  }
  std::memcpy(b->stage.p + fb + tb + vb, fix_attr.data(), (size_t)cnt * AW * 8);
  if (sql) std::memcpy(b->stage.p + fb + tb + vb + ab, fix_sql.data(), fix_sql.size() * sizeof(OtlpSqlFix));
  std::memcpy(b->stage.p + fixb, strs.data(), strs.size());
  HIP_TRY(hipMemcpyAsync(fixdev.p, b->stage.p, fixb, hipMemcpyHostToDevice, st));
  if (!strs.empty())
    HIP_TRY(hipMemcpyAsync(b->arena.p + str_base, b->stage.p + fixb, strs.size(), hipMemcpyHostToDevice, st));
  OtlpFixArgs fa{};
  fa.n = cnt;
  fa.n_attr_keys = K;
  fa.attr_words = AW;
  fa.fix_attr = reinterpret_cast<const uint64_t*>(fixdev.p + fb + tb + vb);
  fa.n_spans = n;
  fa.fix = reinterpret_cast<const OtlpFix*>(fixdev.p);
  fa.fix_type = fixdev.p + fb;
  fa.fix_val = reinterpret_cast<const uint64_t*>(fixdev.p + fb + tb);
  set_span_columns(fa, c);
  launch_otlp_fix(fa, st);
  HIP_TRY(hipGetLastError());
  if (sql) {
    launch_otlp_sqlop_fix(reinterpret_cast<const OtlpSqlFix*>(fixdev.p + fb + tb + vb + ab), cnt,
                          const_cast<uint8_t*>(c.db_flags), const_cast<ose_strref*>(c.db_query), st);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));   // fixdev and the staging are reused / freed
  return 0;
}

int decode(Engine* e, const uint8_t* pb, size_t len, hipStream_t st, OtlpBatchImpl* b, bool host_scopes = false,
           bool host_res = false) {
  int rc;
  OtlpEngine* o = otlp_engine(e, rc);
  if (!o) return rc;
  if (len > 0xFFFFFFF0ull) return fail(OSE_ERANGE, "OTLP ingest: message beyond the 4 GiB arena range");
  using clk = std::chrono::steady_clock;
  auto t0 = clk::now();
  auto lap = [&](int k) {
    const auto t = clk::now();
    b->t_ms[k] = std::chrono::duration<double, std::milli>(t - t0).count();
    t0 = t;
  };
  for (double& x : b->t_ms) x = 0;
  for (int k = 0; k < 8; k++)
    if (k != 4 && k != 5) b->walk_info[k] = 0;   // (the redo flags are the outer call's)
  // engine option otlp_sqlop: db_flags / db_query / res_sql_ok are decoded too
  const bool sql = e->has_sqlop && e->option(Engine::kOptOtlpSqlop);
  // engine option otlp_condattr: odigosconditionalattributes' columns are decoded too
  const bool ca = e->has_condattr && e->option(Engine::kOptOtlpCondattr);
  b->ca_on = false;
  // engine option otlp_url_full: the Path of url.full / http.url is parsed on the GPU
  const bool url_full = e->has_url && e->option(Engine::kOptOtlpUrlFull);
  b->url_full_counts[0] = b->url_full_counts[1] = 0;
  // the walk: TracesData and ResourceSpans on the host, ScopeSpans up to
  // 64 KB on the GPU (engine option otlp_host_scopes: all on the host)
  // (otlp_host_resources: ResourceSpans on the host, ScopeSpans on the
  // GPU; without it only the TracesData chain is walked on the host)
  const bool gpu_scopes = !host_scopes && !e->option(Engine::kOptOtlpHostScopes);
  const bool gpu_res = gpu_scopes && !host_res && !e->option(Engine::kOptOtlpHostResources);
  bool pinned = false, redo = false;
  if ((rc = upload_message(b, pb, len, st, &pinned))) return rc;
  lap(0);
  Walked w;
  OtlpResArgs ra{};
  uint64_t R = 0, S = 0, n = 0;
  if ((rc = walk_records(o, b, pb, len, st, gpu_scopes, gpu_res, !pinned, sql, w, &ra, &R, &S, &redo))) return rc;
  if (redo) {   // a malformed record: the host walk reports it
    b->walk_info[5] = 1;
    return decode(e, pb, len, st, b, false, true);
  }
  lap(1);
  if ((rc = walk_scopes(e, o, b, pb, len, st, gpu_scopes, gpu_res, w, &ra, R, &S, &n, &redo))) return rc;
  if (redo) {   // a scope needs the host walk: all on the host
    b->walk_info[4] = 1;
    return decode(e, pb, len, st, b, true, true);
  }
  uint64_t* span_ref = nullptr;
  HostList hl;
  UrlFullCols uf;
  if ((rc = column_slab(o, b, w, ra, gpu_scopes, gpu_res, sql, n, R, S, st, &span_ref, &hl, url_full ? &uf : nullptr)))
    return rc;
  lap(2);
  uint32_t cnt = 0;
  if ((rc = span_kernels(e, o, b, n, span_ref, hl, sql, ca, url_full ? &uf : nullptr, st, &cnt))) return rc;
  lap(3);
  std::vector<uint32_t> list;   // the host pass's spans: none without a count
  if (cnt && (rc = host_pass(o, b, pb, w, gpu_res, sql, cnt, hl.list, st, list))) return rc;
  if (b->url_full_counts[1] && (rc = url_full_unescape(b, uf, st))) return rc;
  if (ca && (rc = condattr_finish(e, b, pb, list, hl.list, st))) return rc;
  if (cnt) lap(4);
  return 0;
}
}  // namespace

// ---- batches of the groupbytrace store (gbt_host.cpp) ---------------------------
void otlp_batch_view(const ose_otlp_batch* bb, OtlpBatchView* v) {
  const auto* b = reinterpret_cast<const OtlpBatchImpl*>(bb);
  *v = OtlpBatchView{};
  v->e = b->e;
  v->cols = &b->cols;
  v->released = b->released;
  v->d_spans = b->d_spans;
  v->res_on_device = b->res_on_device;
  v->d_res_ref = b->d_res_ref;
  v->d_scope_ref = b->d_scope_ref;
  v->h_res_ref = b->lay.res_ref.data();
  v->h_res_n = b->lay.res_ref.size();
  v->h_scope_ref = b->lay.scope_ref.data();
  v->h_scope_n = b->lay.scope_ref.size();
}

ose_otlp_batch* otlp_released_new(Engine* e) {
  auto* b = new OtlpBatchImpl();
  b->e = e;
  b->released = true;
  return reinterpret_cast<ose_otlp_batch*>(b);
}

void otlp_released_delete(ose_otlp_batch* bb) { delete reinterpret_cast<OtlpBatchImpl*>(bb); }

int otlp_released_arena(ose_otlp_batch* bb, size_t bytes, uint8_t** p) {
  auto* b = reinterpret_cast<OtlpBatchImpl*>(bb);
  if (int rc = b->arena.need(bytes)) return rc;
  *p = b->arena.p;
  return 0;
}

void otlp_released_set(ose_otlp_batch* bb, const ose_columns& cols, const OtlpReleasedLayout& l) {
  auto* b = reinterpret_cast<OtlpBatchImpl*>(bb);
  b->cols = cols;
  b->pb = nullptr;   // the host encoder's copy is made on demand (ose_otlp_encode)
  b->pb_len = 0;
  b->span_ref.clear();
  b->lay = OtlpLayout{};
  b->layout_on_host = false;
  b->res_on_device = true;
  b->scopes_dev = true;
  b->d_spans = b->d_span_ref = const_cast<uint64_t*>(l.spans);
  b->d_span0 = const_cast<uint32_t*>(l.span0);
  b->d_hdr = const_cast<uint64_t*>(l.hdr);
  b->d_schema = const_cast<uint64_t*>(l.schema);
  b->d_res_ref = const_cast<uint64_t*>(l.res_ref);
  b->d_res_scope0 = const_cast<uint32_t*>(l.res_scope0);
  b->d_scope_ref = const_cast<uint64_t*>(l.scope_ref);
}

}  // namespace ose

using namespace ose;

extern "C" {

int ose_otlp_decode(ose_engine* eng, const void* pb, size_t len, void* hip_stream, ose_otlp_batch** out) {
  if (!eng || (!pb && len) || !out) return fail(OSE_EINVAL, "NULL argument");
  Engine* e = reinterpret_cast<Engine*>(eng);
  if (int rc = bind_device(e)) return rc;
  OtlpBatchImpl* b = nullptr;
  {
    // released batches keep their (grow-only) buffers: no allocation per call
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->otlp_pool.empty()) {
      b = static_cast<OtlpBatchImpl*>(e->otlp_pool.back());
      e->otlp_pool.pop_back();
    }
  }
  if (!b) b = new OtlpBatchImpl();
  b->e = e;
  b->walk_info[4] = b->walk_info[5] = 0;
  const int rc = decode(e, static_cast<const uint8_t*>(pb), len, static_cast<hipStream_t>(hip_stream), b);
  if (rc) {
    (void)hipStreamSynchronize(static_cast<hipStream_t>(hip_stream));   // no copy may outlive the buffers
    delete b;
    return rc;
  }
  engine_retain(e);
  *out = reinterpret_cast<ose_otlp_batch*>(b);
  return 0;
}

// Test seam (CPU): url_full.hpp's host instantiation on one string.  out[4]:
// the outcome (0 error, 1 empty, 2 in place, 3 decoded), the Path's sub-range
// (offset, length) and its decoded length; `decoded` (may be NULL, else at
// least len bytes) takes the Path's bytes: the sub-range as it is, or unescaped.
int osehost_url_full_parse(const char* s, size_t len, uint32_t out[4], uint8_t* decoded) {
  if ((!s && len) || !out) return fail(OSE_EINVAL, "NULL argument");
  if (len > 0xFFFFFFF0ull) return fail(OSE_ERANGE, "osehost_url_full_parse: string beyond 4 GiB");
  urlfull::ViewSrc src{s};
  const urlfull::Result r = urlfull::parse(src, 0, (uint32_t)len);
  out[0] = r.outcome;
  out[1] = r.off;
  out[2] = r.len;
  out[3] = r.dec_len;
  if (decoded && r.outcome == urlfull::kDecoded) urlfull::unescape_into(src, r.off, r.len, decoded);
  else if (decoded && r.outcome == urlfull::kInPlace) std::memcpy(decoded, s + r.off, r.len);
  return 0;
}

// Test seam (CPU): the structural walk alone, for a pipeline config
// {"odigossampling": ..., "odigosurltemplate": ..., "odigostrafficmetrics": ...};
// the arrays as JSON, NULL on an error (osehost_last_error)
char* osehost_otlp_walk(const char* cfg_json, const uint8_t* pb, size_t len) {
  try {
    Json cfg = parse_json(cfg_json);
    UrlTemplateConfig url;
    SamplingConfig sampling;
    TrafficMetricsConfig traffic;
    std::string err;
    const Json* ju = cfg.get("odigosurltemplate");
    const Json* js = cfg.get("odigossampling");
    const Json* jt = cfg.get("odigostrafficmetrics");
    if (ju && err.empty()) err = decode_url_config(*ju, url);
    if (js && err.empty()) err = decode_sampling_config(*js, sampling);
    if (jt && err.empty()) err = decode_traffic_config(*jt, traffic);
    ColumnizeCtx ctx;
    if (err.empty()) err = ctx.build(ju ? &url : nullptr, js ? &sampling : nullptr, jt ? &traffic : nullptr);
    Walked w;
    ResCache cache;
    const bool gpu_scopes = cfg.get("gpu_scopes") != nullptr;   // the walk ose_otlp_decode runs (ScopeSpans left to the GPU)
    if (cfg.get("warm") && err.empty()) {   // diagnostics: time a walk whose resource cache is filled
      Walked w0;
      if (!walk(ctx, cache, pb, len, w0, gpu_scopes)) err = w0.err;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (err.empty() && !walk(ctx, cache, pb, len, w, gpu_scopes)) err = w.err;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!err.empty()) { fail(OSE_EINVAL, err); return nullptr; }
    if (cfg.get("timing_only")) {   // diagnostics: the walk's wall time only
      std::string out = "{\"walk_ms\":" + std::to_string(ms) + ",\"spans\":" + std::to_string(w.span_ref.size()) + "}";
      char* r = static_cast<char*>(std::malloc(out.size() + 1));
      std::memcpy(r, out.c_str(), out.size() + 1);
      return r;
    }
    auto arr = [](const auto& v) {
      Json a = Json::array();
      for (auto x : v) a.push(Json::number(std::to_string((uint64_t)x)));
      return a;
    };
    Json o = Json::object();
    o.set("span_ref", arr(w.span_ref));
    o.set("span_res", arr(w.span_res));
    o.set("span_scope", arr(w.span_scope));
    o.set("res_svc", arr(w.res_svc));
    o.set("res_svc_str", arr(w.res_svc_str));
    o.set("res_attrset", arr(w.res_attrset));
    o.set("res_size", arr(w.res_size));
    o.set("res_ok", arr(w.res_ok));
    o.set("scope_size", arr(w.scope_size));
    o.set("scope_res", arr(w.scope_res));
    o.set("n_sets", Json::number(std::to_string(w.sets.size())));
    std::string out;
    dump_json(out, o);
    char* r = static_cast<char*>(std::malloc(out.size() + 1));
    std::memcpy(r, out.c_str(), out.size() + 1);
    return r;
  } catch (const std::exception& ex) {
    fail(OSE_EINVAL, ex.what());
    return nullptr;
  }
}

int ose_otlp_download(const ose_otlp_batch* bb, const ose_columns* dst) {
  if (!bb || !dst) return fail(OSE_EINVAL, "NULL argument");
  const auto* b = reinterpret_cast<const OtlpBatchImpl*>(bb);
  if (int rc = bind_device(b->e)) return rc;
  return download_columns(b->cols, dst);
}

const ose_columns* ose_otlp_columns(const ose_otlp_batch* bb) {
  return bb ? &reinterpret_cast<const OtlpBatchImpl*>(bb)->cols : nullptr;
}

int ose_otlp_timings(const ose_otlp_batch* bb, double* ms5) {
  if (!bb || !ms5) return fail(OSE_EINVAL, "NULL argument");
  if (reinterpret_cast<const OtlpBatchImpl*>(bb)->released)
    return fail(OSE_ENOTSUP, "ose_otlp_timings: a batch released by a groupbytrace store was not decoded");
  std::memcpy(ms5, reinterpret_cast<const OtlpBatchImpl*>(bb)->t_ms, sizeof(double) * 5);
  return 0;
}

int ose_otlp_url_full_counts(const ose_otlp_batch* bb, uint64_t out[2]) {
  if (!bb || !out) return fail(OSE_EINVAL, "NULL argument");
  const auto* b = reinterpret_cast<const OtlpBatchImpl*>(bb);
  if (b->released)
    return fail(OSE_ENOTSUP, "ose_otlp_url_full_counts: a batch released by a groupbytrace store was not decoded");
  out[0] = b->url_full_counts[0];
  out[1] = b->url_full_counts[1];
  return 0;
}

uint32_t ose_otlp_host_spans(const ose_otlp_batch* bb) {
  if (bb && reinterpret_cast<const OtlpBatchImpl*>(bb)->released)
    return (uint32_t)fail(OSE_ENOTSUP, "ose_otlp_host_spans: a batch released by a groupbytrace store was not decoded");
  return bb ? reinterpret_cast<const OtlpBatchImpl*>(bb)->host_spans : 0;
}

int ose_otlp_walk_info(const ose_otlp_batch* bb, uint32_t out[8]) {
  if (!bb || !out) return fail(OSE_EINVAL, "NULL argument");
  if (reinterpret_cast<const OtlpBatchImpl*>(bb)->released)
    return fail(OSE_ENOTSUP, "ose_otlp_walk_info: a batch released by a groupbytrace store was not decoded");
  std::memcpy(out, reinterpret_cast<const OtlpBatchImpl*>(bb)->walk_info, sizeof(uint32_t) * 8);
  return 0;
}

int ose_otlp_attrset(const ose_otlp_batch* bb, uint32_t k, char* json, size_t cap) {
  if (!bb || !json) return fail(OSE_EINVAL, "NULL argument");
  const auto* b = reinterpret_cast<const OtlpBatchImpl*>(bb);
  if (b->released)   // its res_attrset ids are the caller's stable ids (ose_gbt_add_otlp's attrset_map)
    return fail(OSE_ENOTSUP, "ose_otlp_attrset: a released batch's attribute set ids are the caller's");
  if (k >= b->attrsets.size()) return fail(OSE_EINVAL, "attribute set index out of range");
  Json o = Json::object();
  for (auto& kv : b->attrsets[k]) o.set(kv.first, Json::str(kv.second));
  std::string s;
  dump_json(s, o);
  if (s.size() + 1 > cap) return fail(OSE_ERANGE, "buffer too small");
  std::memcpy(json, s.c_str(), s.size() + 1);
  return 0;
}

const ose_condattr_columns* ose_otlp_condattr_columns(const ose_otlp_batch* bb) {
  if (!bb) return nullptr;
  const auto* b = reinterpret_cast<const OtlpBatchImpl*>(bb);
  return b->ca_on && !b->released ? &b->ca : nullptr;
}

int ose_otlp_condattr_download(const ose_otlp_batch* bb, const ose_condattr_columns* dst) {
  if (!bb || !dst) return fail(OSE_EINVAL, "NULL argument");
  const auto* b = reinterpret_cast<const OtlpBatchImpl*>(bb);
  if (!b->ca_on || b->released)
    return fail(OSE_EINVAL, "ose_otlp_condattr_download: the batch was decoded with the engine option otlp_condattr off");
  if (int rc = bind_device(b->e)) return rc;
  const ose_condattr_columns& c = b->ca;
  const uint64_t n = c.n_spans, R = c.n_resources, S = c.n_scopes, K = b->ca_keys;
  struct F { const void* src; const void* dst; size_t bytes; };
  const F fs[] = {
      {c.arena, dst->arena, c.arena_bytes}, {c.scope, dst->scope, 4 * n}, {c.scope_resource, dst->scope_resource, 4 * S},
      {c.scope_name, dst->scope_name, 8 * S}, {c.span_has, dst->span_has, K * n}, {c.span_val, dst->span_val, 8 * K * n},
      {c.span_kv_size, dst->span_kv_size, 4 * K * n}, {c.scope_has, dst->scope_has, K * S},
      {c.scope_val, dst->scope_val, 8 * K * S}, {c.res_has, dst->res_has, K * R}, {c.res_val, dst->res_val, 8 * K * R},
      {c.span_size, dst->span_size, 4 * n},
  };
  for (auto& f : fs)
    if (f.src && f.dst && f.bytes) HIP_TRY(hipMemcpy(const_cast<void*>(f.dst), f.src, f.bytes, hipMemcpyDefault));
  return 0;
}

void ose_otlp_release(ose_otlp_batch* bb) {
  if (!bb) return;
  LastErrorScope keep("ose_otlp_release");
  auto* b = reinterpret_cast<OtlpBatchImpl*>(bb);
  if (b->released) return;   // the store's: freed by the next release's reuse or ose_gbt_destroy
  Engine* e = b->e;
  (void)bind_device(e);
  bool pooled = false;
  if (!e->closed.load()) {
    std::lock_guard<std::mutex> g(e->mu);
    if (e->otlp_pool.size() < 16) {
      e->otlp_pool.push_back(b);
      pooled = true;
    }
  }
  if (!pooled) delete b;
  engine_unref(e);
}

}  // extern "C"
