// condattr_device.hpp — odigosconditionalattributes (processor.go:26-137,
// traces) over the columns of ose_condattr_columns: the value hash, the
// compare, the scope step and the span step, for the device
// (condattr_kernel.hip) and the host (osehost_condattr_span, the sanitizer
// driver): one source.
//
// The host compiles the config into one blob (condattr_host.cpp):
//   Header | Rule[] | Key[] | Target[] | List[] | Action[] | Slot[] | strings
// Every rule has an open-addressing table of its configured values (linear
// probing, load <= 1/2, so a probe run ends at an empty slot); equal action
// lists are stored once.  The strings start 16-byte aligned and are followed
// by 32 readable bytes, so the aligned 16-byte loads of ByteReader stay
// inside the blob.
//
// Per-target state lives in the output columns themselves: src[t * n + i] is
// written OSE_CA_KEEP first and re-read by the lane that wrote it whenever a
// later action, rule or default asks whether the span has the name or what
// its value is.  A lane only ever reads back its own stores, the columns are
// key-major (consecutive lanes, consecutive addresses), no register is
// indexed by a runtime target number and no bound on targets follows.
#pragma once
#include <cstdint>

#include "../../include/odigos_amd.h"

#if defined(__HIP__)   // compiled as HIP (condattr_kernel.hip); plain C++ elsewhere
#define OSE_CA_HD __host__ __device__ inline
#else
#define OSE_CA_HD inline
#endif

namespace ose {
namespace condattr {

constexpr uint32_t kNone = 0xFFFFFFFFu;
enum : uint32_t { kRuleScopeName = 0, kRuleKey = 1 };          // processor.go:59
enum : uint32_t { kActNone = 0, kActStatic = 1, kActFrom = 2 };   // :79, :87; neither: the action does nothing

struct Header {
  uint32_t n_rules, n_keys, n_targets, n_lists;
  uint32_t rules_off, keys_off, targets_off, lists_off, actions_off, slots_off, strings_off, string_bytes;   // byte offsets
  uint32_t dflt_off, dflt_len;   // global_default in the strings
  uint32_t pad[2];
};
struct Rule {
  uint32_t kind, key;          // key: kRuleKey only
  uint32_t slot0, mask;        // the rule's slots [slot0, slot0 + mask + 1)
  uint32_t n_values, max_len;  // a longer check string matches nothing
  uint32_t pad[2];
};
struct Slot { uint32_t hash, off, len, list; };   // off == kNone: empty
struct Key { uint32_t off, len, target, pad; };
struct Target { uint32_t key, name_len, dflt, pad; };   // dflt: the name is not "" (factory.go:69)
struct List { uint32_t first, count; };
struct Action { uint32_t kind, target, a, b; };   // kActStatic: value {off a, len b}; kActFrom: key a

struct View {
  const Header* h;
  const Rule* rules;
  const Key* keys;
  const Target* targets;
  const List* lists;
  const Action* actions;
  const Slot* slots;
  const uint8_t* strings;
};
OSE_CA_HD View view(const uint8_t* blob) {
  View v;
  v.h = reinterpret_cast<const Header*>(blob);
  v.rules = reinterpret_cast<const Rule*>(blob + v.h->rules_off);
  v.keys = reinterpret_cast<const Key*>(blob + v.h->keys_off);
  v.targets = reinterpret_cast<const Target*>(blob + v.h->targets_off);
  v.lists = reinterpret_cast<const List*>(blob + v.h->lists_off);
  v.actions = reinterpret_cast<const Action*>(blob + v.h->actions_off);
  v.slots = reinterpret_cast<const Slot*>(blob + v.h->slots_off);
  v.strings = blob + v.h->strings_off;
  return v;
}

// plain bytes in host memory
struct HostBytes {
  const uint8_t* p;
  OSE_CA_HD uint32_t at(uint32_t i) const { return p[i]; }
};
struct HostEnv {
  using Reader = HostBytes;
  static OSE_CA_HD Reader reader(const uint8_t* p) { return HostBytes{p}; }
};

// protobuf framing of tests/otlp_gogo.py: tag (< 16) + varint length + payload
OSE_CA_HD uint32_t sov(uint64_t x) { return 1u + (uint32_t)((63 - __builtin_clzll((unsigned long long)(x | 1))) / 7); }
OSE_CA_HD uint64_t field_len(uint64_t l) { return 1 + sov(l) + l; }
// Span.attributes entry of PutStr(key, value): KeyValue{key omitted when "",
// value always framed, the string oneof emitted even when empty}
OSE_CA_HD uint64_t kv_framed(uint32_t key_len, uint32_t val_len) {
  return field_len((key_len ? field_len(key_len) : 0) + field_len(field_len(val_len)));
}

// FNV-1a over the bytes
template <class Reader>
OSE_CA_HD uint32_t hash_bytes(Reader& rd, uint32_t n) {
  uint32_t h = 2166136261u;
  for (uint32_t i = 0; i < n; i++) h = (h ^ rd.at(i)) * 16777619u;
  return h;
}
OSE_CA_HD uint32_t hash_bytes_host(const uint8_t* p, uint32_t n) {
  uint32_t h = 2166136261u;
  for (uint32_t i = 0; i < n; i++) h = (h ^ p[i]) * 16777619u;
  return h;
}

template <class Reader>
OSE_CA_HD bool equal_bytes(Reader& rd, const uint8_t* s, uint32_t n) {
  for (uint32_t i = 0; i < n; i++)
    if (rd.at(i) != s[i]) return false;
  return true;
}

// rule.NewAttributeValueConfigurations[check] (processor.go:75, :109): the
// action list of the exact bytes, or kNone
template <class Reader>
OSE_CA_HD uint32_t lookup(const View& v, const Rule& r, Reader& rd, uint32_t n) {
  if (r.n_values == 0 || n > r.max_len) return kNone;
  const uint32_t h = hash_bytes(rd, n);
  uint32_t p = h & r.mask;
  for (uint32_t step = 0; step <= r.mask; step++, p = (p + 1) & r.mask) {
    const Slot s = v.slots[r.slot0 + p];
    if (s.off == kNone) return kNone;
    if (s.hash == h && s.len == n && equal_bytes(rd, v.strings + s.off, n)) return s.list;
  }
  return kNone;
}

// scratch layout: [n_rules][n_scopes] action lists, then [n_targets][n_scopes]
// "the scope and its resource both have the target's name" (:82-85, :91-94)
OSE_CA_HD uint64_t scratch_words(const Header& h, uint32_t n_scopes) {
  return ((uint64_t)h.n_rules + h.n_targets) * n_scopes;
}

// What depends on the scope alone.  Scope-name rules: the matched list.  Key
// rules: the list of a span without the key, from the scope's attribute, else
// the resource's, else "" (:66-75; the "" is looked up like any value).
template <class Env>
OSE_CA_HD void scope_step(const View& v, const ose_condattr_columns& c, uint32_t* scratch, uint32_t s) {
  const uint64_t S = c.n_scopes, R = c.n_resources;
  const uint32_t res = c.scope_resource[s];
  const uint32_t nr = v.h->n_rules, nt = v.h->n_targets;
  for (uint32_t r = 0; r < nr; r++) {
    const Rule rule = v.rules[r];
    ose_strref ref{0, 0};
    if (rule.kind == kRuleScopeName) {
      ref = c.scope_name[s];
    } else if (c.scope_has[rule.key * S + s]) {
      ref = c.scope_val[rule.key * S + s];
    } else if (c.res_has[rule.key * R + res]) {
      ref = c.res_val[rule.key * R + res];
    }
    auto rd = Env::reader(c.arena + ref.off);
    scratch[r * S + s] = lookup(v, rule, rd, ref.len);
  }
  for (uint32_t t = 0; t < nt; t++) {
    const uint64_t k = v.targets[t].key;
    scratch[(nr + t) * S + s] = (c.scope_has[k * S + s] && c.res_has[k * R + res]) ? 1u : 0u;
  }
}

// spanAttributes.Get(key) as the span is now: what an earlier put left in the
// output columns, else the span's own column
struct Cur {
  uint32_t has, src;
  ose_strref ref;
};
OSE_CA_HD bool cur_has(const View& v, const ose_condattr_columns& c, const ose_condattr_outputs& o, uint64_t i, uint32_t k) {
  const uint32_t t = v.keys[k].target;
  if (t != kNone && o.src[t * c.n_spans + i] != OSE_CA_KEEP) return true;
  return c.span_has[k * c.n_spans + i] != 0;
}
OSE_CA_HD Cur cur_get(const View& v, const ose_condattr_columns& c, const ose_condattr_outputs& o, uint64_t i, uint32_t k) {
  const uint32_t t = v.keys[k].target;
  if (t != kNone) {
    const uint32_t sc = o.src[t * c.n_spans + i];
    if (sc != OSE_CA_KEEP) return Cur{1u, sc, o.val[t * c.n_spans + i]};
  }
  Cur x{c.span_has[k * c.n_spans + i], OSE_CA_ARENA, ose_strref{0, 0}};
  if (x.has) x.ref = c.span_val[k * c.n_spans + i];
  return x;
}

// processSpan (processor.go:43-53) for span i
template <class Env>
OSE_CA_HD void span_step(const View& v, const ose_condattr_columns& c, const ose_condattr_outputs& o,
                         const uint32_t* scratch, uint64_t i) {
  const uint64_t n = c.n_spans, S = c.n_scopes;
  const uint32_t s = c.scope[i];
  const uint32_t nr = v.h->n_rules, nt = v.h->n_targets;
  for (uint32_t t = 0; t < nt; t++) o.src[t * n + i] = OSE_CA_KEEP;
  for (uint32_t r = 0; r < nr; r++) {
    const Rule rule = v.rules[r];
    uint32_t list = scratch[r * S + s];
    if (rule.kind == kRuleKey) {
      const Cur x = cur_get(v, c, o, i, rule.key);   // the span's own value comes first (:66-72)
      if (x.has) {
        auto rd = Env::reader((x.src == OSE_CA_CONFIG ? v.strings : c.arena) + x.ref.off);
        list = lookup(v, rule, rd, x.ref.len);
      }
    }
    if (list == kNone) continue;
    const List L = v.lists[list];
    for (uint32_t a = 0; a < L.count; a++) {
      const Action act = v.actions[L.first + a];
      uint32_t vsrc;
      ose_strref vref;
      if (act.kind == kActStatic) {          // value != "" comes before from_field (:79, :111)
        vsrc = OSE_CA_CONFIG;
        vref = ose_strref{act.a, act.b};
      } else if (act.kind == kActFrom) {     // the span's attributes only (:88, :118)
        const Cur f = cur_get(v, c, o, i, act.a);
        if (!f.has) continue;
        vsrc = f.src;
        vref = f.ref;
      } else {
        continue;
      }
      const uint32_t t = act.target;
      const bool present = cur_has(v, c, o, i, v.targets[t].key);
      // scope-name rules put iff the span lacks the name (:113, :119); the
      // others unless span, scope and resource all have it (:80-85, :89-95)
      const bool put = rule.kind == kRuleScopeName ? !present : !(present && scratch[(nr + t) * S + s]);
      if (put) {
        o.src[t * n + i] = (uint8_t)vsrc;
        o.val[t * n + i] = vref;
      }
    }
  }
  // setDefaultValueAttributes (:129-137)
  for (uint32_t t = 0; t < nt; t++) {
    const Target tg = v.targets[t];
    if (tg.dflt && !cur_has(v, c, o, i, tg.key)) {
      o.src[t * n + i] = OSE_CA_CONFIG;
      o.val[t * n + i] = ose_strref{v.h->dflt_off, v.h->dflt_len};
    }
  }
  if (o.span_size_out && c.span_size) {
    uint64_t sz = c.span_size[i];
    for (uint32_t t = 0; t < nt; t++) {
      if (o.src[t * n + i] == OSE_CA_KEEP) continue;
      const Target tg = v.targets[t];
      sz += kv_framed(tg.name_len, o.val[t * n + i].len);
      if (c.span_has[tg.key * n + i]) sz -= c.span_kv_size[tg.key * n + i];
    }
    o.span_size_out[i] = (uint32_t)sz;
  }
}

}  // namespace condattr
}  // namespace ose
