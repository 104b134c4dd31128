// sqlop_host.cpp — odigossqldboperationprocessor: the launches of the SQLOP
// stage and of the size stage's spans pass after it (sqlop_kernel.hip), and
// the host seam of the shared classifier.
#include "engine_internal.hpp"
#include "kernels.hpp"
#include "sqlop_device.hpp"

namespace ose {

// DBOperationProcessor.processTraces (processor.go:30-78): one plain launch
// on the caller's stream, every span classified whatever keep says (the
// reference runs after odigossampling removed the dropped spans; their
// sql_op bytes are never applied).
int run_sqlop(Engine* e, const ose_columns* c, const ose_outputs* o, hipStream_t st) {
  if (!e->has_sqlop) return fail(OSE_EINVAL, "odigossqldboperationprocessor is not configured on this engine");
  if (!c->db_flags || !c->db_query || !c->resource || !o->sql_op)
    return fail(OSE_EINVAL, "SQLOP stage needs db_flags, db_query, resource and sql_op");
  if (c->n_spans == 0) return 0;
  if (!c->arena) return fail(OSE_EINVAL, "SQLOP stage needs the arena");
  SqlOpArgs a{};
  a.n_spans = c->n_spans;
  a.arena = c->arena;
  a.db_flags = c->db_flags;
  a.db_query = c->db_query;
  a.resource = c->resource;
  a.res_sql_ok = c->res_sql_ok;
  a.sql_op = o->sql_op;
  return e->timed("sqlop_kernel", st, [&] { launch_sqlop(a, st); });
}

// SIZE after SQLOP / APPLY_SQLOP: what prepare_size does not ask for
int check_sqlop_size(const ose_columns* c, const ose_outputs* o) {
  if (c->n_spans && (!c->name_len || !o->sql_op)) return fail(OSE_EINVAL, "SIZE after SQLOP needs name_len and sql_op");
  return 0;
}

// run_size_tail with sqlop_size_span_kernel as the spans pass
int run_sqlop_size_tail(Engine* e, const SizeKernelArgs& a, const uint8_t* sql_op, hipStream_t st) {
  SqlSizeArgs sa{};
  sa.sz = a;
  sa.sql_op = sql_op;
  if (const int rc = e->timed("sqlop_size_span_kernel", st, [&] { launch_sqlop_size_spans(sa, st); })) return rc;
  return run_size_scopes(e, a, st);
}

}  // namespace ose

// Test seam, no device: the OSE_SQLOP_* code of DetectSQLOperationName
// (processor.go:84-115) for the bytes, from the classifier the kernel's
// general path compiles.
extern "C" uint32_t osehost_sqlop_detect(const char* bytes, size_t len) {
  if (!bytes || len == 0 || len > 0xFFFFFFFFull) return ose::sqlop::kNone;
  ose::sqlop::HostBytes rd{reinterpret_cast<const uint8_t*>(bytes)};
  return ose::sqlop::detect(rd, (uint32_t)len);
}
