// columnize.cpp — see columnize.hpp.
#include "columnize.hpp"

#include <algorithm>
#include <cstring>

#include "host.hpp"
#include "urlparse.hpp"

namespace ose {

bool workload_key(const AttrMap& attrs, std::string& key) {
  const Value* ns = attrs.Get("k8s.namespace.name");
  if (!ns || ns->type != Value::TStr) return false;
  struct { const char* attr; const char* kind; } order[] = {
      {"k8s.deployment.name", "deployment"}, {"k8s.statefulset.name", "statefulset"}, {"k8s.daemonset.name", "daemonset"}};
  for (auto& o : order) {
    const Value* v = attrs.Get(o.attr);
    if (!v) continue;
    if (v->type != Value::TStr) return false;
    key = ns->s + "/" + o.kind + "/" + v->s;
    return true;
  }
  return false;
}

std::set<std::string> workload_set(const MatchProperties& mp) {
  std::set<std::string> s;
  for (auto& w : mp.k8s_workloads) {
    std::string k = w.kind;
    for (auto& c : k) c = (char)std::tolower((unsigned char)c);
    s.insert(w.namespace_ + "/" + k + "/" + w.name);
  }
  return s;
}

std::string ColumnizeCtx::build(const UrlTemplateConfig* url, const SamplingConfig* sampling,
                                const TrafficMetricsConfig* traffic, const SqlOpConfig* sql) {
  if (sql) {
    sqlop = true;
    if (sql->has_exclude) sql_exclude = sql->exclude_language;
  }
  if (url) {
    has_exclude = url->exclude.has_value();
    has_include = url->include.has_value();
    url_filter = has_exclude || has_include;
    if (has_exclude) excl = workload_set(*url->exclude);
    if (has_include) incl = workload_set(*url->include);
  }
  if (traffic) traffic_keys = traffic->res_attributes_keys;
  if (sampling) {
    services = intern_services(*sampling);
    for (auto* lvl : {&sampling->global_rules, &sampling->service_rules, &sampling->endpoint_rules})
      for (auto& r : *lvl)
        if (r.rtype == RuleType::SpanAttribute) {
          attr_preds.emplace_back();
          std::string e = attr_preds.back().compile(r.attr);
          if (!e.empty()) return e;
        }
    attr_plan = plan_attr_rules(*sampling);
  }
  return "";
}

ResourceCols columnize_resource(const ColumnizeCtx& c, const AttrMap& ra) {
  ResourceCols r;
  // service ids (latency.go:51-56 AsString; servicename.go:38-42 Str)
  const Value* sv = ra.Get("service.name");
  if (sv) {
    const std::string as = sv->AsString();
    // span_attribute rules whose service this resource is (spanattribute.go:130-132)
    r.attr_res.assign((c.attr_preds.size() + 63) / 64, 0);
    for (size_t k = 0; k < c.attr_preds.size(); k++)
      if (c.attr_preds[k].service() == as) r.attr_res[k / 64] |= 1ull << (k % 64);
    auto it = c.services.find(as);
    if (it != c.services.end()) {
      r.svc = it->second;
      if (sv->type == Value::TStr) r.svc_str = it->second;
    }
  }
  // include/exclude (odigosurltemplateprocessor/processor.go:76-85)
  if (c.url_filter) {
    std::string key;
    const bool has_key = workload_key(ra, key);
    if (c.has_exclude && has_key && c.excl.count(key)) r.url_ok = 0;
    if (c.has_include && !(has_key && c.incl.count(key))) r.url_ok = 0;
  }
  // shouldExcludeLanguage (odigossqldboperationprocessor/processor.go:119-143):
  // with a non-empty list, a resource without telemetry.sdk.language is
  // excluded, and so is one whose AsString value is listed
  if (c.sqlop && !c.sql_exclude.empty()) {
    const Value* lang = ra.Get("telemetry.sdk.language");
    if (!lang) {
      r.sql_ok = 0;
    } else {
      const std::string lv = lang->AsString();
      if (std::find(c.sql_exclude.begin(), c.sql_exclude.end(), lv) != c.sql_exclude.end()) r.sql_ok = 0;
    }
  }
  // attributeSetFromResource (odigostrafficmetrics/processor.go:60-69)
  std::map<std::string, std::string> set;
  for (auto& k : c.traffic_keys)
    if (const Value* v = ra.Get(k)) set[k] = v->Str();
  r.attrset.assign(set.begin(), set.end());
  return r;
}

void columnize_span(const ColumnizeCtx& c, const Span& sp, const std::vector<uint64_t>& attr_res, const ProtoSizer& sizer,
                    SpanCols& o) {
  o.hi = o.lo = 0;
  for (int k = 0; k < 8; k++) { o.hi = o.hi << 8 | sp.trace_id[k]; o.lo = o.lo << 8 | sp.trace_id[8 + k]; }
  o.start = sp.start;
  o.end = sp.end;
  o.status = status_column(sp.status_code);
  o.kind = (uint8_t)std::min<int32_t>(std::max<int32_t>(sp.kind, 0), 255);
  o.span_size = (uint32_t)sizer.span(sp);
  o.name_len = (uint32_t)sp.name.size();
  // span_attribute: the "json" conditions here, the others from the key columns on the GPU
  const size_t W = std::max<size_t>(1, (c.attr_preds.size() + 63) / 64);
  o.attr_match.assign(W, 0);
  for (size_t w = 0; w < attr_res.size() && w < c.attr_plan.host_mask.size(); w++)
    for (uint64_t m = attr_res[w] & c.attr_plan.host_mask[w]; m; m &= m - 1) {
      const size_t k = 64 * w + (size_t)__builtin_ctzll(m);
      if (const Value* av = sp.attrs.Get(c.attr_preds[k].key()))
        if (c.attr_preds[k].eval(*av)) o.attr_match[w] |= 1ull << (k % 64);
    }
  const size_t nk = c.attr_plan.keys.size();
  o.attr_type.assign(nk, OSE_ATTR_ABSENT);
  o.attr_val.assign(nk, 0);
  o.attr_str.assign(nk, std::string_view());
  for (size_t k = 0; k < nk; k++) {
    const Value* av = sp.attrs.Get(c.attr_plan.keys[k]);
    if (!av) continue;
    switch (av->type) {
      case Value::TStr: o.attr_type[k] = OSE_ATTR_STR; o.attr_str[k] = av->s; break;
      case Value::TInt: o.attr_type[k] = OSE_ATTR_INT; o.attr_val[k] = (uint64_t)av->i; break;
      case Value::TDouble: o.attr_type[k] = OSE_ATTR_DOUBLE; std::memcpy(&o.attr_val[k], &av->d, 8); break;
      case Value::TBool: o.attr_type[k] = OSE_ATTR_BOOL; o.attr_val[k] = av->b ? 1 : 0; break;
      default: o.attr_type[k] = OSE_ATTR_OTHER; break;
    }
  }
  // the keys the processors read, picked up in one pass over the span's
  // attributes (each the first of its key, as pcommon.Map.Get finds it)
  const Value *route = nullptr, *method = nullptr, *method_old = nullptr, *url_tmpl = nullptr, *url_path = nullptr,
              *target = nullptr, *url_full = nullptr, *http_url = nullptr;
  auto first = [](const Value*& slot, const Value& v) {
    if (!slot) slot = &v;
  };
  for (auto& e : sp.attrs.kv) {
    const std::string& k = e.first;
    switch (k.size()) {
      case 8:
        if (k == "url.path") first(url_path, e.second);
        else if (k == "url.full") first(url_full, e.second);
        else if (k == "http.url") first(http_url, e.second);
        break;
      case 10:
        if (k == "http.route") first(route, e.second);
        break;
      case 11:
        if (k == "http.method") first(method_old, e.second);
        else if (k == "http.target") first(target, e.second);
        break;
      case 12:
        if (k == "url.template") first(url_tmpl, e.second);
        break;
      case 19:
        if (k == "http.request.method") first(method, e.second);
        break;
      default:
        break;
    }
  }
  // sampling: AsString(http.route) (latency.go:64-68)
  o.has_route = route != nullptr;
  if (route && route->type == Value::TStr) {
    o.route = route->s;
  } else {
    o.route_own = route ? route->AsString() : std::string();
    o.route = o.route_own;
  }
  auto as_view = [&](const Value* v) -> std::string_view {
    if (v->type == Value::TStr) return v->s;
    o.path_own = v->AsString();
    return o.path_own;
  };
  // urltemplate (processor.go:98-147, 235-287)
  uint8_t f = 0;
  o.path = std::string_view();
  const Value* m = method ? method : method_old;
  if (m) {
    f |= OSE_URL_HAS_METHOD;
    if (m->type == Value::TStr ? sp.name == m->s : sp.name == m->AsString()) f |= OSE_URL_NAME_EQ_METHOD;
    if (const Value* tv = sp.kind == OSE_KIND_CLIENT ? url_tmpl : route) {
      if (tv->type != Value::TStr) f |= OSE_URL_TGT_NONSTR;
      else f |= tv->s.empty() ? OSE_URL_TGT_STR_EMPTY : OSE_URL_TGT_STR;
    }
    if (const Value* p = url_path) {
      f |= OSE_URL_PATH_RAW;
      o.path = as_view(p);
    } else if (const Value* p = target) {
      f |= OSE_URL_PATH_TARGET;
      o.path = as_view(p);
    } else {
      const Value* fu = url_full ? url_full : http_url;
      std::string path;
      if (fu && go_url_parse_path(fu->AsString(), path)) {
        f |= OSE_URL_PATH_RAW;
        o.path_own = std::move(path);
        o.path = o.path_own;
      }
    }
  }
  o.url_flags = f;
  // odigossqldboperationprocessor (processor.go:52-64)
  o.db_flags = 0;
  o.db_query = std::string_view();
  if (c.sqlop) {
    const Value* q = sp.attrs.Get("db.query.text");
    if (q) {
      o.db_flags |= OSE_DB_HAS_QUERY;
      if (q->type == Value::TStr) {
        o.db_query = q->s;
      } else {
        o.db_query_own = q->AsString();
        o.db_query = o.db_query_own;
      }
    }
    if (sp.attrs.Get("db.operation.name")) o.db_flags |= OSE_DB_HAS_OPNAME;
  }
}

// processSpan's reads (odigosconditionalattributes/processor.go:43-126) as
// columns: per key, Map.Get on the span, scope and resource maps (:68, :80-84)
// and AsString of what it finds (:69, :90), plus the scope names (:36).
void condattr_lookup(const std::vector<std::string>& keys, const AttrMap& m, size_t row, size_t rows, std::string& arena,
                     size_t arena_base, const ProtoSizer& sizer, uint8_t* has, ose_strref* val, uint32_t* kv_size) {
  for (size_t k = 0; k < keys.size(); k++) {
    const Value* v = m.Get(keys[k]);
    if (!v) continue;
    const size_t at = arena.size();
    if (v->type == Value::TStr) arena += v->s;
    else arena += v->AsString();
    has[k * rows + row] = 1;
    val[k * rows + row] = ose_strref{(uint32_t)(arena_base + at), (uint32_t)(arena.size() - at)};
    if (kv_size) kv_size[k * rows + row] = (uint32_t)field_len(sizer.key_value(keys[k], *v));
  }
}

void columnize_condattr(const std::vector<std::string>& keys, size_t n_targets, const Traces& t, const ProtoSizer& sizer,
                        CondAttrHostCols& o) {
  const size_t K = keys.size(), R = t.resource_spans.size();
  size_t S = 0, N = 0;
  for (auto& rs : t.resource_spans) {
    S += rs.scope_spans.size();
    for (auto& ss : rs.scope_spans) N += ss.spans.size();
  }
  std::string arena;
  auto pad = [](size_t x) { return std::max<size_t>(x, 1); };   // data() never NULL
  o.scope.assign(pad(N), 0);
  o.scope_resource.assign(pad(S), 0);
  o.scope_name.assign(pad(S), ose_strref{0, 0});
  o.span_has.assign(pad(K * N), 0);
  o.span_val.assign(pad(K * N), ose_strref{0, 0});
  o.span_kv_size.assign(pad(K * N), 0);
  o.scope_has.assign(pad(K * S), 0);
  o.scope_val.assign(pad(K * S), ose_strref{0, 0});
  o.res_has.assign(pad(K * R), 0);
  o.res_val.assign(pad(K * R), ose_strref{0, 0});
  size_t i = 0, si = 0;
  for (size_t ri = 0; ri < R; ri++) {
    const ResourceSpans& rs = t.resource_spans[ri];
    condattr_lookup(keys, rs.resource_attrs, ri, R, arena, 0, sizer, o.res_has.data(), o.res_val.data(), nullptr);
    for (auto& ss : rs.scope_spans) {
      o.scope_resource[si] = (uint32_t)ri;
      o.scope_name[si] = ose_strref{(uint32_t)arena.size(), (uint32_t)ss.scope_name.size()};
      arena += ss.scope_name;
      condattr_lookup(keys, ss.scope_attrs, si, S, arena, 0, sizer, o.scope_has.data(), o.scope_val.data(), nullptr);
      for (auto& sp : ss.spans) {
        o.scope[i] = (uint32_t)si;
        condattr_lookup(keys, sp.attrs, i, N, arena, 0, sizer, o.span_has.data(), o.span_val.data(), o.span_kv_size.data());
        i++;
      }
      si++;
    }
  }
  o.arena.assign((arena.size() + 15) / 16 * 16 + 16, 0);
  if (!arena.empty()) std::memcpy(o.arena.data(), arena.data(), arena.size());
  o.src.assign(pad(n_targets * N), 0);
  o.val.assign(pad(n_targets * N), ose_strref{0, 0});
  o.span_size_out.assign(pad(N), 0);
  o.cols = ose_condattr_columns{};
  o.cols.n_spans = N;
  o.cols.n_resources = (uint32_t)R;
  o.cols.n_scopes = (uint32_t)S;
  o.cols.arena_bytes = arena.size();
  o.cols.arena = o.arena.data();
  o.cols.scope = o.scope.data();
  o.cols.scope_resource = o.scope_resource.data();
  o.cols.scope_name = o.scope_name.data();
  o.cols.span_has = o.span_has.data();
  o.cols.span_val = o.span_val.data();
  o.cols.span_kv_size = o.span_kv_size.data();
  o.cols.scope_has = o.scope_has.data();
  o.cols.scope_val = o.scope_val.data();
  o.cols.res_has = o.res_has.data();
  o.cols.res_val = o.res_val.data();
  o.outs = ose_condattr_outputs{};
  o.outs.src = o.src.data();
  o.outs.val = o.val.data();
  o.outs.span_size_out = o.span_size_out.data();
}

}  // namespace ose
