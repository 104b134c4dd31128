// gen_otlp.cpp — a serialized TracesData for the OTLP ingest benchmark and
// tests (bench/test infrastructure, part of libosegen): the resources,
// spans, times, statuses, kinds, paths and routes of a generated batch
// (gen_batch.cpp), written as OTLP trace.proto messages with the attributes
// an HTTP instrumentation sets, encoded as pdata's marshaler writes them
// (what a node collector's OTLP exporter sends the gateway: proto3 defaults
// omitted, ids and Status always framed); resources are encoded in parallel
// chunks (TracesData is a concatenation of ResourceSpans fields).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/odigos_amd.h"

namespace {

void put_varint(std::string& o, uint64_t v) {
  while (v >= 0x80) { o += (char)(v | 0x80); v >>= 7; }
  o += (char)v;
}
void put_tag(std::string& o, uint32_t field, uint32_t wt) { put_varint(o, ((uint64_t)field << 3) | wt); }
void put_bytes(std::string& o, uint32_t field, const char* p, size_t n) {
  put_tag(o, field, 2);
  put_varint(o, n);
  o.append(p, n);
}
void put_str(std::string& o, uint32_t field, const std::string& s) { put_bytes(o, field, s.data(), s.size()); }
void put_fixed64(std::string& o, uint32_t field, uint64_t v) {
  put_tag(o, field, 1);
  char b[8];
  std::memcpy(b, &v, 8);
  o.append(b, 8);
}
void put_msg(std::string& o, uint32_t field, const std::string& m) { put_bytes(o, field, m.data(), m.size()); }
// KeyValue{key, AnyValue{string_value}} / {int_value}
void kv_str(std::string& o, uint32_t field, const char* k, const char* v, size_t vl) {
  std::string av, kv;
  put_bytes(av, 1, v, vl);
  put_bytes(kv, 1, k, std::strlen(k));
  put_msg(kv, 2, av);
  put_msg(o, field, kv);
}
void kv_int(std::string& o, uint32_t field, const char* k, int64_t v) {
  std::string av, kv;
  put_tag(av, 3, 0);
  put_varint(av, (uint64_t)v);
  put_bytes(kv, 1, k, std::strlen(k));
  put_msg(kv, 2, av);
  put_msg(o, field, kv);
}
uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
const char* kMethod[] = {"GET", "POST", "PUT", "DELETE"};
// db.query.text of the spans that carry one (osegen_otlp_sql): statements a
// database instrumentation records, some in lower case or after blanks, one
// the processor does not know
const char* kQuery[] = {
    "SELECT id, name, email FROM users WHERE id = ?",
    "select * from orders o join items i on i.order_id = o.id where o.customer_id = ? order by o.created_at desc limit 50",
    "INSERT INTO events (id, kind, payload, created_at) VALUES (?, ?, ?, now())",
    "  UPDATE accounts SET balance = balance - ? WHERE id = ?",
    "DELETE FROM sessions WHERE expires_at < ?",
    "\n\tSELECT count(*) FROM audit_log WHERE tenant = ? AND at > ?",
    "EXPLAIN ANALYZE SELECT 1",
    "CREATE INDEX idx_items_order ON items (order_id)",
};

struct Res { uint64_t first, count; };
// the InstrumentationScope names to draw from (osegen_otlp_scoped): resource r's
// scope takes names[mix(r) % n]; none: the net/http instrumentation's name
struct ScopeNames {
  const char* bytes = nullptr;
  const uint32_t* lens = nullptr;
  std::vector<uint64_t> offs;
};

// sql_every != 0: one span in sql_every also carries a db.query.text (its last attribute)
// url_full_ppm: that share (in millionths) of the spans with a method and a
// path source carries url.full alone in its place, as a client instrumentation
// under the stable HTTP conventions sends it: scheme, host and port, the same
// path, a query; a tenth of them with one more, escaped, segment
void encode_resources(const ose_columns* c, const std::vector<Res>& res, size_t r0, size_t r1, std::string& out,
                      uint32_t sql_every, const ScopeNames& names, uint32_t url_full_ppm) {
  std::string rs, sc, sp, tmp;
  for (size_t r = r0; r < r1; r++) {
    rs.clear();
    {   // Resource
      std::string resm;
      char name[32];
      const uint32_t svc = c->res_svc[r] == OSE_NONE ? 99 : c->res_svc[r];
      std::snprintf(name, sizeof name, "svc-%02u", svc);
      kv_str(resm, 1, "service.name", name, std::strlen(name));
      kv_str(resm, 1, "k8s.namespace.name", "default", 7);
      kv_str(resm, 1, "k8s.deployment.name", name, std::strlen(name));   // what k8sattributes adds
      char pod[32];
      std::snprintf(pod, sizeof pod, "pod-%u", c->res_attrset[r] % 4);
      kv_str(resm, 1, "k8s.pod.name", pod, std::strlen(pod));
      kv_str(resm, 1, "telemetry.sdk.language", "go", 2);
      put_msg(rs, 1, resm);
    }
    sc.clear();
    {   // InstrumentationScope
      std::string scm;
      if (names.offs.empty()) {
        put_str(scm, 1, "go.opentelemetry.io/contrib/instrumentation/net/http");
      } else {
        const size_t k = (size_t)(mix(r ^ 0x5C09E) % names.offs.size());
        put_str(scm, 1, std::string(names.bytes + names.offs[k], names.lens[k]));
      }
      put_str(scm, 2, "0.53.0");
      put_msg(sc, 1, scm);
    }
    for (uint64_t i = res[r].first; i < res[r].first + res[r].count; i++) {
      sp.clear();
      char id[16];
      for (int k = 0; k < 8; k++) id[k] = (char)(c->trace_id[2 * i] >> (56 - 8 * k));
      for (int k = 0; k < 8; k++) id[8 + k] = (char)(c->trace_id[2 * i + 1] >> (56 - 8 * k));
      put_bytes(sp, 1, id, 16);
      const uint64_t h = mix(i ^ c->trace_id[2 * i]);
      std::memcpy(id, &h, 8);
      put_bytes(sp, 2, id, 8);
      if (h & 3) {
        const uint64_t h2 = mix(h);
        std::memcpy(id, &h2, 8);
        put_bytes(sp, 4, id, 8);
      } else {
        put_bytes(sp, 4, id, 0);   // pdata frames an empty parent id
      }
      const uint8_t f = c->url_flags[i];
      const char* method = kMethod[h >> 62];
      if (f & OSE_URL_NAME_EQ_METHOD) {
        put_str(sp, 5, method);
      } else {
        tmp.assign("op-");
        tmp.append(std::to_string(h % 100000));
        put_str(sp, 5, tmp);
      }
      if (c->kind[i]) { put_tag(sp, 6, 0); put_varint(sp, c->kind[i]); }
      if (c->start_ns[i]) put_fixed64(sp, 7, c->start_ns[i]);
      if (c->end_ns[i]) put_fixed64(sp, 8, c->end_ns[i]);
      if (f & OSE_URL_HAS_METHOD) kv_str(sp, 9, "http.request.method", method, std::strlen(method));
      const ose_strref rt = c->route[i];
      const uint32_t tgt = f & OSE_URL_TGT_MASK;
      if (c->kind[i] == OSE_KIND_SERVER && (rt.len || tgt == OSE_URL_TGT_STR_EMPTY))
        kv_str(sp, 9, "http.route", (const char*)c->arena + rt.off, rt.len);
      if (c->kind[i] == OSE_KIND_CLIENT && tgt == OSE_URL_TGT_STR) kv_str(sp, 9, "url.template", "/t/{id}", 7);
      const ose_strref p = c->path[i];
      if (url_full_ppm && (f & OSE_URL_HAS_METHOD) && (f & OSE_URL_PATH_MASK) != OSE_URL_PATH_NONE &&
          mix(h ^ 0xF0115) % 1000000 < url_full_ppm) {
        const char* path = (const char*)c->arena + p.off;
        const void* q = std::memchr(path, '?', p.len);
        tmp.assign("https://api.internal.svc:8443");
        tmp.append(path, q ? (size_t)((const char*)q - path) : p.len);
        if (mix(h ^ 0xE5CA9) % 10 == 0) tmp.append("/caf%C3%A9%20menu");
        tmp.append("?page=2&sort=asc");
        kv_str(sp, 9, "url.full", tmp.data(), tmp.size());
      } else if ((f & OSE_URL_PATH_MASK) == OSE_URL_PATH_RAW) {
        kv_str(sp, 9, "url.path", (const char*)c->arena + p.off, p.len);
      } else if ((f & OSE_URL_PATH_MASK) == OSE_URL_PATH_TARGET) {
        kv_str(sp, 9, "http.target", (const char*)c->arena + p.off, p.len);
      }
      if (f & OSE_URL_HAS_METHOD) {   // what an HTTP instrumentation adds next to them
        kv_int(sp, 9, "http.response.status_code", c->status[i] == OSE_STATUS_ERROR ? 500 : 200);
        static const char kUa[] = "Mozilla/5.0 (X11; Linux x86_64) odigos-bench/1.0";
        kv_str(sp, 9, "server.address", "api.internal.svc", 16);
        kv_str(sp, 9, "network.protocol.version", "1.1", 3);
        kv_str(sp, 9, "user_agent.original", kUa, sizeof kUa - 1);
      }
      if (sql_every && mix(h ^ 0x5C1) % sql_every == 0) {
        const char* q = kQuery[mix(h ^ 0xD8) % (sizeof kQuery / sizeof kQuery[0])];
        kv_str(sp, 9, "db.query.text", q, std::strlen(q));
      }
      {   // Status: non-nullable, always framed
        std::string st;
        if (c->status[i]) {
          put_tag(st, 3, 0);
          put_varint(st, c->status[i]);
        }
        put_msg(sp, 15, st);
      }
      put_msg(sc, 2, sp);
    }
    put_msg(rs, 2, sc);
    put_msg(out, 1, rs);
  }
}

}  // namespace

extern "C" {

// TracesData bytes of the batch `cols` (as osegen_columns returns it: spans
// in resource order, one scope per resource).  *len receives the size;
// free with osegen_otlp_free.  osegen_otlp_sql: the same with a db.query.text
// on one span in sql_every (0: none), for the odigossqldboperationprocessor legs.
// osegen_otlp_scoped: the same with every resource's scope name drawn from
// n_names names (their bytes back to back in `names`, lengths in name_lens),
// for the odigosconditionalattributes legs.  osegen_otlp_url_full: the same as
// osegen_otlp_sql with url.full alone on url_full_ppm millionths of the spans
// that have a method and a path source (encode_resources).
static char* otlp_bytes(const ose_columns* c, int threads, uint64_t* len, uint32_t sql_every, const ScopeNames& names,
                        uint32_t url_full_ppm = 0) {
  std::vector<Res> res(c->n_resources, Res{0, 0});
  for (uint64_t i = 0; i < c->n_spans; i++) {
    const uint32_t r = c->resource[i];
    if (res[r].count == 0) res[r].first = i;
    res[r].count++;
  }
  if (threads < 1) threads = 1;
  const size_t R = res.size();
  std::vector<std::string> parts((size_t)threads);
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++)
    th.emplace_back([&, t]() { encode_resources(c, res, R * t / threads, R * (t + 1) / threads, parts[t], sql_every, names, url_full_ppm); });
  for (auto& x : th) x.join();
  uint64_t total = 0;
  for (auto& p : parts) total += p.size();
  char* out = static_cast<char*>(std::malloc(total ? total : 1));
  uint64_t off = 0;
  for (auto& p : parts) {
    std::memcpy(out + off, p.data(), p.size());
    off += p.size();
  }
  *len = total;
  return out;
}

char* osegen_otlp_sql(const ose_columns* c, int threads, uint64_t* len, uint32_t sql_every) {
  return otlp_bytes(c, threads, len, sql_every, ScopeNames{});
}

char* osegen_otlp_scoped(const ose_columns* c, int threads, uint64_t* len, uint32_t sql_every, const char* names,
                         const uint32_t* name_lens, uint32_t n_names) {
  ScopeNames sn;
  sn.bytes = names;
  sn.lens = name_lens;
  uint64_t off = 0;
  for (uint32_t k = 0; k < n_names; k++) {
    sn.offs.push_back(off);
    off += name_lens[k];
  }
  return otlp_bytes(c, threads, len, sql_every, sn);
}

char* osegen_otlp_url_full(const ose_columns* c, int threads, uint64_t* len, uint32_t sql_every, uint32_t url_full_ppm) {
  return otlp_bytes(c, threads, len, sql_every, ScopeNames{}, url_full_ppm);
}

char* osegen_otlp(const ose_columns* c, int threads, uint64_t* len) { return osegen_otlp_sql(c, threads, len, 0); }

void osegen_otlp_free(char* p) { std::free(p); }

}  // extern "C"
