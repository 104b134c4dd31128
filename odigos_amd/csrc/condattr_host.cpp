// condattr_host.cpp — odigosconditionalattributes: the config compiler, the
// entry points ose_condattr_process / ose_condattr_process_device and the
// engine's queries, and the host seams of the shared steps
// (condattr_device.hpp).
#include "condattr_host.hpp"

#include <array>
#include <cstring>
#include <map>

#include "condattr_device.hpp"
#include "engine_internal.hpp"
#include "kernels.hpp"

namespace ose {

namespace {
size_t up16(size_t x) { return (x + 15) / 16 * 16; }
}  // namespace

int compile_condattr(const CondAttrConfig& cfg, CondAttrCompiled& out) {
  using namespace condattr;
  out = CondAttrCompiled{};
  std::string strings;
  std::map<std::string, uint32_t> interned;
  auto intern = [&](const std::string& s) -> uint32_t {
    auto it = interned.find(s);
    if (it != interned.end()) return it->second;
    const uint32_t off = (uint32_t)strings.size();
    strings += s;
    interned.emplace(s, off);
    return off;
  };
  std::map<std::string, uint32_t> key_id;
  auto key_of = [&](const std::string& name) -> uint32_t {
    auto it = key_id.find(name);
    if (it != key_id.end()) return it->second;
    const uint32_t k = (uint32_t)out.keys.size();
    key_id.emplace(name, k);
    out.keys.push_back(name);
    out.key_target.push_back(OSE_NONE);
    return k;
  };
  auto target_of = [&](const std::string& name) -> uint32_t {
    const uint32_t k = key_of(name);
    if (out.key_target[k] == OSE_NONE) {
      out.key_target[k] = (uint32_t)out.target_key.size();
      out.target_key.push_back(k);
    }
    return out.key_target[k];
  };
  std::vector<Rule> rules;
  std::vector<List> lists;
  std::vector<Action> actions;
  std::vector<Slot> slots;
  std::map<std::vector<std::array<uint32_t, 4>>, uint32_t> list_ids;
  uint64_t total_value_bytes = 0;
  for (auto& rule : cfg.rules)
    for (auto& kv : rule.values) total_value_bytes += kv.first.size() + 64 * (kv.second.size() + 1);
  if (total_value_bytes + cfg.global_default.size() >= (1ull << 31))
    return fail(OSE_ENOTSUP, "odigosconditionalattributes: the compiled tables index with 32 bits; this config passes 2 GiB");
  for (auto& rule : cfg.rules) {
    Rule r{};
    r.kind = rule.field_to_check == "instrumentation_scope.name" ? kRuleScopeName : kRuleKey;   // processor.go:59
    if (r.kind == kRuleKey) r.key = key_of(rule.field_to_check);
    uint32_t cap = 1;
    while ((uint64_t)cap < 2 * (uint64_t)rule.values.size()) cap <<= 1;
    r.slot0 = (uint32_t)slots.size();
    r.mask = cap - 1;
    r.n_values = (uint32_t)rule.values.size();
    slots.resize(slots.size() + cap, Slot{0, kNone, 0, kNone});
    for (auto& kv : rule.values) {   // std::map: byte order
      std::vector<std::array<uint32_t, 4>> la;
      for (auto& act : kv.second) {
        Action a{};
        if (!act.value.empty()) {
          a.kind = kActStatic;
          a.target = target_of(act.new_attribute);
          a.a = intern(act.value);
          a.b = (uint32_t)act.value.size();
        } else if (!act.from_field.empty()) {
          a.kind = kActFrom;
          a.a = key_of(act.from_field);
          a.target = target_of(act.new_attribute);
        } else {
          a.kind = kActNone;   // does nothing; its name still gets the default (factory.go:68-71)
          a.target = target_of(act.new_attribute);
        }
        la.push_back({a.kind, a.target, a.a, a.b});
      }
      auto it = list_ids.find(la);
      if (it == list_ids.end()) {
        it = list_ids.emplace(la, (uint32_t)lists.size()).first;
        lists.push_back(List{(uint32_t)actions.size(), (uint32_t)la.size()});
        for (auto& x : la) actions.push_back(Action{x[0], x[1], x[2], x[3]});
      }
      Slot sl;
      sl.hash = hash_bytes_host(reinterpret_cast<const uint8_t*>(kv.first.data()), (uint32_t)kv.first.size());
      sl.off = intern(kv.first);
      sl.len = (uint32_t)kv.first.size();
      sl.list = it->second;
      r.max_len = std::max(r.max_len, sl.len);
      uint32_t p = sl.hash & r.mask;
      while (slots[r.slot0 + p].off != kNone) p = (p + 1) & r.mask;
      slots[r.slot0 + p] = sl;
    }
    rules.push_back(r);
  }
  std::vector<Key> keys(out.keys.size());
  for (size_t k = 0; k < keys.size(); k++)
    keys[k] = Key{intern(out.keys[k]), (uint32_t)out.keys[k].size(), out.key_target[k], 0};
  std::vector<Target> targets(out.target_key.size());
  for (size_t t = 0; t < targets.size(); t++) {
    const std::string& name = out.keys[out.target_key[t]];
    targets[t] = Target{out.target_key[t], (uint32_t)name.size(), name.empty() ? 0u : 1u, 0};
  }
  Header h{};
  h.n_rules = (uint32_t)rules.size();
  h.n_keys = (uint32_t)keys.size();
  h.n_targets = (uint32_t)targets.size();
  h.n_lists = (uint32_t)lists.size();
  h.dflt_off = intern(cfg.global_default);
  h.dflt_len = (uint32_t)cfg.global_default.size();
  size_t off = up16(sizeof(Header));
  auto place = [&](size_t bytes) { const size_t o = off; off = up16(off + bytes); return (uint32_t)o; };
  h.rules_off = place(rules.size() * sizeof(Rule));
  h.keys_off = place(keys.size() * sizeof(Key));
  h.targets_off = place(targets.size() * sizeof(Target));
  h.lists_off = place(lists.size() * sizeof(List));
  h.actions_off = place(actions.size() * sizeof(Action));
  h.slots_off = place(slots.size() * sizeof(Slot));
  h.strings_off = place(strings.size());
  h.string_bytes = (uint32_t)strings.size();
  if ((uint64_t)off + 32 >= (1ull << 32))
    return fail(OSE_ENOTSUP, "odigosconditionalattributes: the compiled tables index with 32 bits; this config passes 4 GiB");
  out.blob.assign(off + 32, 0);
  uint8_t* b = out.blob.data();
  std::memcpy(b, &h, sizeof h);
  auto put = [&](uint32_t o, const void* p, size_t bytes) { if (bytes) std::memcpy(b + o, p, bytes); };
  put(h.rules_off, rules.data(), rules.size() * sizeof(Rule));
  put(h.keys_off, keys.data(), keys.size() * sizeof(Key));
  put(h.targets_off, targets.data(), targets.size() * sizeof(Target));
  put(h.lists_off, lists.data(), lists.size() * sizeof(List));
  put(h.actions_off, actions.data(), actions.size() * sizeof(Action));
  put(h.slots_off, slots.data(), slots.size() * sizeof(Slot));
  put(h.strings_off, strings.data(), strings.size());
  out.n_rules = h.n_rules;
  out.strings_off = h.strings_off;
  out.string_bytes = h.string_bytes;
  return 0;
}

int refuse_condattr(const char* entry) {
  return fail(OSE_ENOTSUP, std::string(entry) + " do not take OSE_STAGE_CONDATTR: odigosconditionalattributes runs through "
                                                "ose_condattr_process / ose_condattr_process_device");
}

void release_condattr(Engine* e) {
  if (e->condattr_blob_dev) (void)hipFree(e->condattr_blob_dev);
  if (e->condattr_pin) (void)hipHostFree(e->condattr_pin);
  if (e->condattr_stage) (void)hipFree(e->condattr_stage);
  if (e->condattr_slots_dev) (void)hipFree(e->condattr_slots_dev);
  e->condattr_slots_dev = nullptr;
  e->condattr_blob_dev = nullptr;
  e->condattr_pin = e->condattr_stage = nullptr;
}

// The table otlp_condattr_kernel finds a span's attribute keys in: open
// addressing on the key bytes' FNV-1a (the hash of condattr_device.hpp), load
// <= 1/2 so that a probe run ends at an empty slot, and the set of key lengths.
int build_condattr_keytab(Engine* e) {
  std::lock_guard<std::mutex> g(e->condattr_mu);
  if (e->condattr_slots_dev) return 0;
  if (const int brc = bind_device(e)) return brc;
  const std::vector<std::string>& keys = e->condattr_tab.keys;
  uint32_t cap = 2;
  while ((uint64_t)cap < 2 * (uint64_t)keys.size()) cap <<= 1;
  std::vector<OtlpCaSlot> slots(cap, OtlpCaSlot{0, condattr::kNone});
  uint64_t lens = 0;
  for (size_t k = 0; k < keys.size(); k++) {
    const uint32_t h = condattr::hash_bytes_host(reinterpret_cast<const uint8_t*>(keys[k].data()), (uint32_t)keys[k].size());
    uint32_t p = h & (cap - 1);
    while (slots[p].key != condattr::kNone) p = (p + 1) & (cap - 1);
    slots[p] = OtlpCaSlot{h, (uint32_t)k};
    lens |= 1ull << std::min<size_t>(keys[k].size(), 63);
  }
  void* d = nullptr;
  HIP_TRY(hipMalloc(&d, slots.size() * sizeof(OtlpCaSlot)));
  const hipError_t he = hipMemcpy(d, slots.data(), slots.size() * sizeof(OtlpCaSlot), hipMemcpyHostToDevice);
  if (he != hipSuccess) {
    (void)hipFree(d);
    return fail(OSE_EDEVICE, std::string("engine option otlp_condattr: ") + hipGetErrorString(he));
  }
  e->condattr_slot_mask = cap - 1;
  e->condattr_key_lens = lens;
  e->condattr_slots_dev = d;
  return 0;
}

namespace {

int check_args(const Engine* e, const ose_condattr_columns* c, const ose_condattr_outputs* o) {
  if (!e->has_condattr) return fail(OSE_EINVAL, "odigosconditionalattributes is not configured on this engine");
  if (!c || !o) return fail(OSE_EINVAL, "columns and outputs are required");
  if (c->n_spans == 0) return 0;
  if (c->n_scopes == 0 || c->n_resources == 0) return fail(OSE_EINVAL, "CONDATTR: spans need scopes and resources");
  if (!c->scope || !c->scope_resource || !c->scope_name) return fail(OSE_EINVAL, "CONDATTR needs scope, scope_resource and scope_name");
  if (c->arena_bytes > 0xFFFFFFFFull) return fail(OSE_ERANGE, "CONDATTR: the arena passes 4 GiB");
  if (c->arena_bytes && !c->arena) return fail(OSE_EINVAL, "CONDATTR needs the arena");
  if (!e->condattr_tab.keys.empty() &&
      (!c->span_has || !c->span_val || !c->scope_has || !c->scope_val || !c->res_has || !c->res_val))
    return fail(OSE_EINVAL, "CONDATTR needs span_has, span_val, scope_has, scope_val, res_has and res_val");
  if (!e->condattr_tab.target_key.empty() && (!o->src || !o->val)) return fail(OSE_EINVAL, "CONDATTR needs src and val");
  if (o->span_size_out && (!c->span_size || (!e->condattr_tab.target_key.empty() && !c->span_kv_size)))
    return fail(OSE_EINVAL, "span_size_out needs span_size and span_kv_size");
  return 0;
}

int launch_both(Engine* e, const ose_condattr_columns* c, const ose_condattr_outputs* o, hipStream_t st) {
  CondAttrArgs a{};
  a.blob = e->condattr_blob_dev;
  a.c = *c;
  a.o = *o;
  if (const int rc = e->timed("condattr_scope_kernel", st, [&] { launch_condattr_scopes(a, st); })) return rc;
  return e->timed("condattr_span_kernel", st, [&] { launch_condattr_spans(a, st); });
}

// every index and string ref the kernels follow, checked on the host columns
int check_host_columns(const CondAttrCompiled& tab, const ose_condattr_columns* c) {
  const uint64_t n = c->n_spans, S = c->n_scopes, R = c->n_resources, K = tab.keys.size();
  for (uint64_t i = 0; i < n; i++)
    if (c->scope[i] >= S) return fail(OSE_EINVAL, "CONDATTR: a span's scope is out of range");
  for (uint64_t s = 0; s < S; s++) {
    if (c->scope_resource[s] >= R) return fail(OSE_EINVAL, "CONDATTR: a scope's resource is out of range");
    const ose_strref r = c->scope_name[s];
    if ((uint64_t)r.off + r.len > c->arena_bytes) return fail(OSE_EINVAL, "CONDATTR: a scope name leaves the arena");
  }
  auto refs = [&](const uint8_t* has, const ose_strref* val, uint64_t cnt) {
    for (uint64_t x = 0; x < cnt; x++)
      if (has[x] && (uint64_t)val[x].off + val[x].len > c->arena_bytes) return false;
    return true;
  };
  if (!refs(c->span_has, c->span_val, K * n) || !refs(c->scope_has, c->scope_val, K * S) || !refs(c->res_has, c->res_val, K * R))
    return fail(OSE_EINVAL, "CONDATTR: an attribute value leaves the arena");
  return 0;
}

}  // namespace
}  // namespace ose

using namespace ose;

extern "C" {

int ose_engine_condattr_info(const ose_engine* eng, ose_condattr_info* info) {
  if (!eng || !info) return fail(OSE_EINVAL, "NULL argument");
  const Engine* e = reinterpret_cast<const Engine*>(eng);
  if (!e->has_condattr) return fail(OSE_EINVAL, "odigosconditionalattributes is not configured on this engine");
  info->n_rules = e->condattr_tab.n_rules;
  info->n_keys = (uint32_t)e->condattr_tab.keys.size();
  info->n_targets = (uint32_t)e->condattr_tab.target_key.size();
  info->string_bytes = e->condattr_tab.string_bytes;
  return 0;
}

int ose_engine_condattr_key(const ose_engine* eng, uint32_t k, const char** bytes, uint32_t* len, uint32_t* target) {
  if (!eng || !bytes || !len) return fail(OSE_EINVAL, "NULL argument");
  const Engine* e = reinterpret_cast<const Engine*>(eng);
  if (!e->has_condattr || k >= e->condattr_tab.keys.size()) return fail(OSE_EINVAL, "no such odigosconditionalattributes key");
  *bytes = e->condattr_tab.keys[k].data();
  *len = (uint32_t)e->condattr_tab.keys[k].size();
  if (target) *target = e->condattr_tab.key_target[k];
  return 0;
}

int ose_engine_condattr_string(const ose_engine* eng, const char** bytes, uint32_t* len) {
  if (!eng || !bytes || !len) return fail(OSE_EINVAL, "NULL argument");
  const Engine* e = reinterpret_cast<const Engine*>(eng);
  if (!e->has_condattr) return fail(OSE_EINVAL, "odigosconditionalattributes is not configured on this engine");
  *bytes = reinterpret_cast<const char*>(e->condattr_tab.blob.data() + e->condattr_tab.strings_off);
  *len = e->condattr_tab.string_bytes;
  return 0;
}

uint64_t ose_condattr_scratch_words(const ose_engine* eng, uint32_t n_scopes) {
  if (!eng) return 0;
  const Engine* e = reinterpret_cast<const Engine*>(eng);
  if (!e->has_condattr) return 0;
  return ((uint64_t)e->condattr_tab.n_rules + e->condattr_tab.target_key.size()) * n_scopes;
}

int ose_condattr_process_device(ose_engine* eng, const ose_condattr_columns* cols, const ose_condattr_outputs* outs,
                                void* hip_stream) {
  if (!eng) return fail(OSE_EINVAL, "NULL engine");
  Engine* e = reinterpret_cast<Engine*>(eng);
  if (const int rc = check_args(e, cols, outs)) return rc;
  if (cols->n_spans == 0) return 0;
  if (!outs->scratch && ose_condattr_scratch_words(eng, cols->n_scopes))
    return fail(OSE_EINVAL, "ose_condattr_process_device needs scratch (ose_condattr_scratch_words)");
  if (const int brc = bind_device(e)) return brc;
  return launch_both(e, cols, outs, static_cast<hipStream_t>(hip_stream));
}

int ose_condattr_process(ose_engine* eng, const ose_condattr_columns* cols, const ose_condattr_outputs* outs) {
  if (!eng) return fail(OSE_EINVAL, "NULL engine");
  Engine* e = reinterpret_cast<Engine*>(eng);
  if (const int rc = check_args(e, cols, outs)) return rc;
  if (cols->n_spans == 0) return 0;
  const CondAttrCompiled& tab = e->condattr_tab;
  if (const int rc = check_host_columns(tab, cols)) return rc;
  if (const int brc = bind_device(e)) return brc;
  const uint64_t n = cols->n_spans, S = cols->n_scopes, R = cols->n_resources, K = tab.keys.size(), U = tab.target_key.size();
  const bool sized = outs->span_size_out != nullptr;
  // one slab: the inputs, then the outputs, then the scratch (device only)
  size_t off = 0;
  auto place = [&](size_t bytes) { const size_t o = off; off = up16(off + bytes); return o; };
  const size_t o_arena = place(up16(cols->arena_bytes) + 16);
  const size_t o_scope = place(4 * n), o_sres = place(4 * S), o_sname = place(8 * S);
  const size_t o_shas = place(K * n), o_sval = place(8 * K * n), o_skv = place(cols->span_kv_size ? 4 * K * n : 0);
  const size_t o_chas = place(K * S), o_cval = place(8 * K * S), o_rhas = place(K * R), o_rval = place(8 * K * R);
  const size_t o_size = place(cols->span_size ? 4 * n : 0);
  const size_t in_bytes = off;
  const size_t o_src = place(U * n), o_val = place(8 * U * n), o_out = place(sized ? 4 * n : 0);
  const size_t out_end = off;
  const size_t o_scratch = place(4 * (size_t)ose_condattr_scratch_words(eng, cols->n_scopes));
  const size_t total = off;
  std::lock_guard<std::mutex> g(e->condattr_mu);
  if (e->condattr_pin_cap < out_end) {
    if (e->condattr_pin) HIP_TRY(hipHostFree(e->condattr_pin));
    e->condattr_pin = nullptr;
    e->condattr_pin_cap = 0;
    HIP_TRY(hipHostMalloc(&e->condattr_pin, out_end + out_end / 4, hipHostMallocDefault));
    e->condattr_pin_cap = out_end + out_end / 4;
  }
  if (e->condattr_stage_cap < total) {
    if (e->condattr_stage) HIP_TRY(hipFree(e->condattr_stage));
    e->condattr_stage = nullptr;
    e->condattr_stage_cap = 0;
    HIP_TRY(hipMalloc(&e->condattr_stage, total + total / 4));
    e->condattr_stage_cap = total + total / 4;
  }
  uint8_t* pin = static_cast<uint8_t*>(e->condattr_pin);
  uint8_t* dev = static_cast<uint8_t*>(e->condattr_stage);
  auto cp = [&](size_t o, const void* p, size_t bytes) { if (bytes && p) std::memcpy(pin + o, p, bytes); };
  cp(o_arena, cols->arena, cols->arena_bytes);
  std::memset(pin + o_arena + cols->arena_bytes, 0, up16(cols->arena_bytes) + 16 - cols->arena_bytes);
  cp(o_scope, cols->scope, 4 * n);
  cp(o_sres, cols->scope_resource, 4 * S);
  cp(o_sname, cols->scope_name, 8 * S);
  cp(o_shas, cols->span_has, K * n);
  cp(o_sval, cols->span_val, 8 * K * n);
  if (cols->span_kv_size) cp(o_skv, cols->span_kv_size, 4 * K * n);
  cp(o_chas, cols->scope_has, K * S);
  cp(o_cval, cols->scope_val, 8 * K * S);
  cp(o_rhas, cols->res_has, K * R);
  cp(o_rval, cols->res_val, 8 * K * R);
  if (cols->span_size) cp(o_size, cols->span_size, 4 * n);
  ose_condattr_columns dc = *cols;
  dc.arena = dev + o_arena;
  dc.scope = reinterpret_cast<const uint32_t*>(dev + o_scope);
  dc.scope_resource = reinterpret_cast<const uint32_t*>(dev + o_sres);
  dc.scope_name = reinterpret_cast<const ose_strref*>(dev + o_sname);
  dc.span_has = dev + o_shas;
  dc.span_val = reinterpret_cast<const ose_strref*>(dev + o_sval);
  dc.span_kv_size = cols->span_kv_size ? reinterpret_cast<const uint32_t*>(dev + o_skv) : nullptr;
  dc.scope_has = dev + o_chas;
  dc.scope_val = reinterpret_cast<const ose_strref*>(dev + o_cval);
  dc.res_has = dev + o_rhas;
  dc.res_val = reinterpret_cast<const ose_strref*>(dev + o_rval);
  dc.span_size = cols->span_size ? reinterpret_cast<const uint32_t*>(dev + o_size) : nullptr;
  ose_condattr_outputs dout{};
  dout.src = dev + o_src;
  dout.val = reinterpret_cast<ose_strref*>(dev + o_val);
  dout.span_size_out = sized ? reinterpret_cast<uint32_t*>(dev + o_out) : nullptr;
  dout.scratch = reinterpret_cast<uint32_t*>(dev + o_scratch);
  hipStream_t st = e->take_stream();
  int rc = 0;
  hipError_t he = hipMemcpyAsync(dev, pin, in_bytes, hipMemcpyHostToDevice, st);
  if (he != hipSuccess) rc = fail(OSE_EDEVICE, std::string("CONDATTR upload: ") + hipGetErrorString(he));
  if (!rc) rc = launch_both(e, &dc, &dout, st);
  if (!rc && out_end > in_bytes) {
    he = hipMemcpyAsync(pin + in_bytes, dev + in_bytes, out_end - in_bytes, hipMemcpyDeviceToHost, st);
    if (he != hipSuccess) rc = fail(OSE_EDEVICE, std::string("CONDATTR download: ") + hipGetErrorString(he));
  }
  he = hipStreamSynchronize(st);
  if (!rc && he != hipSuccess) rc = fail(OSE_EDEVICE, std::string("CONDATTR: ") + hipGetErrorString(he));
  e->give_stream(st);
  if (rc) return rc;
  if (U) {
    std::memcpy(outs->src, pin + o_src, U * n);
    std::memcpy(outs->val, pin + o_val, 8 * U * n);
  }
  if (sized) std::memcpy(outs->span_size_out, pin + o_out, 4 * n);
  return 0;
}

// ---- test seams, no device --------------------------------------------

// The section of cfg_json decoded and compiled as ose_engine_create does;
// the codes and messages are ose_engine_create's.
static int compile_section(const char* cfg_json, CondAttrCompiled& tab) {
  Json root;
  try {
    root = parse_json(cfg_json ? cfg_json : "{}");
  } catch (const std::exception& ex) {
    return fail(OSE_EINVAL, ex.what());
  }
  const Json* j = root.is_obj() ? root.get("odigosconditionalattributes") : nullptr;
  if (!j) return fail(OSE_EINVAL, "no odigosconditionalattributes section");
  CondAttrConfig cfg;
  const std::string err = decode_condattr_config(*j, cfg);
  if (!err.empty()) return fail(OSE_EINVAL, err);
  return compile_condattr(cfg, tab);
}

// What ose_engine_condattr_info / _key / _string answer for the config:
// info, then (when keys_json is not NULL) a malloc'ed JSON text
// {"keys": [hex], "key_target": [..], "strings": hex} to free with osehost_free.
int osehost_condattr_compile(const char* cfg_json, ose_condattr_info* info, char** keys_json) {
  CondAttrCompiled tab;
  if (const int rc = compile_section(cfg_json, tab)) return rc;
  if (info) {
    info->n_rules = tab.n_rules;
    info->n_keys = (uint32_t)tab.keys.size();
    info->n_targets = (uint32_t)tab.target_key.size();
    info->string_bytes = tab.string_bytes;
  }
  if (keys_json) {
    auto hex = [](const uint8_t* p, size_t n) {
      static const char* d = "0123456789abcdef";
      std::string s;
      for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
      return s;
    };
    std::string s = "{\"keys\":[";
    for (size_t k = 0; k < tab.keys.size(); k++)
      s += (k ? ",\"" : "\"") + hex(reinterpret_cast<const uint8_t*>(tab.keys[k].data()), tab.keys[k].size()) + "\"";
    s += "],\"key_target\":[";
    for (size_t k = 0; k < tab.keys.size(); k++) s += (k ? "," : "") + std::to_string(tab.key_target[k]);
    s += "],\"strings\":\"" + hex(tab.blob.data() + tab.strings_off, tab.string_bytes) + "\"}";
    char* p = static_cast<char*>(std::malloc(s.size() + 1));
    std::memcpy(p, s.c_str(), s.size() + 1);
    *keys_json = p;
  }
  return 0;
}

// The compiled blob of the config (condattr_device.hpp's layout), malloc'ed:
// what the stand-alone sanitizer driver (tests/fuzz/condattr_san.cpp) runs on.
int osehost_condattr_blob(const char* cfg_json, char** blob, size_t* len) {
  if (!blob || !len) return fail(OSE_EINVAL, "NULL argument");
  CondAttrCompiled tab;
  if (const int rc = compile_section(cfg_json, tab)) return rc;
  char* p = static_cast<char*>(std::malloc(tab.blob.size()));
  std::memcpy(p, tab.blob.data(), tab.blob.size());
  *blob = p;
  *len = tab.blob.size();
  return 0;
}

// The scope step for every scope, then the span step for every span, as the
// kernels run them, on host columns (scratch is the seam's own).
int osehost_condattr_span(const char* cfg_json, const ose_condattr_columns* cols, const ose_condattr_outputs* outs) {
  if (!cols || !outs) return fail(OSE_EINVAL, "NULL argument");
  CondAttrCompiled tab;
  if (const int rc = compile_section(cfg_json, tab)) return rc;
  if (cols->n_spans == 0) return 0;
  if (const int rc = check_host_columns(tab, cols)) return rc;
  const condattr::View v = condattr::view(tab.blob.data());
  std::vector<uint32_t> scratch((size_t)condattr::scratch_words(*v.h, cols->n_scopes) + 1, 0);
  for (uint32_t s = 0; s < cols->n_scopes; s++) condattr::scope_step<condattr::HostEnv>(v, *cols, scratch.data(), s);
  for (uint64_t i = 0; i < cols->n_spans; i++) condattr::span_step<condattr::HostEnv>(v, *cols, *outs, scratch.data(), i);
  return 0;
}

}  // extern "C"
