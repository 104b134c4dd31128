// otlp_encode_host.cpp — the front end of the OTLP re-encode:
// ose_otlp_encode, ose_otlp_encode_condattr and the CPU test seams
// osehost_otlp_encode*.
//
// A decoded batch (otlp_batch.hpp) and the stages' decisions become one
// TracesData per output.  The GPU encoder (encode_gpu: encode_kernel.hip)
// takes the call first; what it declines (OtlpOut::fallback says why), and
// OSE_GROUP_BATCH, go to the host encoder (otlp_encode.cpp encode_traces) with
// the decisions copied into the batch's pinned staging.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "otlp_batch.hpp"
#include "taskpool.hpp"

namespace ose {

// ---- the GPU encoder (encode_kernel.hip) -------------------------------------------
namespace {
// 0 with *host false: *o holds the outputs; 0 with *host true: the host
// encoder takes the call (o->fallback says why); else an error code
// ca (ose_otlp_encode_condattr; sampled, tmpl and sql false): odigosconditionalattributes'
// puts are applied, by the kernels' instances for them.
int encode_gpu(OtlpBatchImpl* b, const ose_outputs* outs, bool sampled, bool tmpl, bool sql, const Router* router,
               hipStream_t st, OtlpOut* o, bool* host, std::vector<uint64_t>* res_off = nullptr,
               const ose_condattr_outputs* ca = nullptr) {
  *host = true;
  if (b->e->option(Engine::kOptEncodeHost)) return 0;   // engine option encode_host: the host encoder always
  if (router && router->pipelines.size() > 63) return 0;   // the host encoder reports it
  const uint32_t ca_T = ca ? (uint32_t)b->e->condattr_tab.target_key.size() : 0;
  if (ca_T > kEncCaTargets) {   // the host encoder has no bound on the targets
    o->fallback = kEncFbCa;
    return 0;
  }
  const uint64_t n = b->cols.n_spans, S = b->cols.n_scopes, R = b->cols.n_resources;
  if (!b->d_spans) return 0;
  const uint32_t n_out = router ? (uint32_t)router->pipelines.size() + 1 : 1;
  const uint32_t tiles = (uint32_t)std::max<uint64_t>(1, (R + kEncTiles - 1) / kEncTiles);
  // workspace
  EncArgs a{};
  const size_t blob = router ? router->dev_blob.size() : 0;
  uint64_t* flags64 = nullptr;
  uint32_t *scope_span0 = nullptr, *res_scope0 = nullptr;
  uint64_t *scope_hdr = nullptr, *scope_schema = nullptr, *res_ref = nullptr;
  uint8_t* routes = nullptr;
  uint64_t* out_base = nullptr;
  std::vector<SlabPart> parts = {
      {(void**)&a.span_out, 4 * n},
      {(void**)&a.scope_body, 8 * S},
      {(void**)&a.res_body, 8 * R},
      {(void**)&a.res_rec, 8 * R},
      {(void**)&a.res_mask, 8 * R},
      {(void**)&a.res_hdr, 8 * R},
      {(void**)&a.res_schema, 8 * R},
      {(void**)&flags64, 8},
      {(void**)&a.tile_sum, 16 * (size_t)n_out * tiles},
      {(void**)&a.off, 8 * (size_t)n_out * R},
      {(void**)&a.out_total, 16 * (size_t)n_out},
      {(void**)&out_base, 8 * (size_t)n_out},
  };
  if (tmpl || sql) parts.push_back({(void**)&a.edit, sizeof(EncEdit) * n});
  if (sql) parts.push_back({(void**)&a.sql_edit, sizeof(EncSqlEdit) * n});
  EncCaArgs ca_a{};
  if (ca) {   // the puts in the workspace (src / val may be host memory), and the new span lengths
    parts.push_back({(void**)&ca_a.ca_src, (size_t)ca_T * n});
    parts.push_back({(void**)&ca_a.ca_val, 8 * (size_t)ca_T * n});
    parts.push_back({(void**)&ca_a.ca_len, 4 * n});
  }
  if (blob) parts.push_back({(void**)&routes, blob});
  // the layout arrays the decoder left on the host go up
  const bool up_scopes = !b->scopes_dev, up_res = !b->res_on_device;
  if (up_scopes) {
    parts.push_back({(void**)&scope_span0, 4 * S});
    parts.push_back({(void**)&scope_hdr, 8 * S});
    parts.push_back({(void**)&scope_schema, 8 * S});
  }
  if (up_res) {
    parts.push_back({(void**)&res_ref, 8 * R});
    parts.push_back({(void**)&res_scope0, 4 * R});
  }
  int rc;
  if ((rc = slab_place(b->eslab, parts))) return rc;
  // host-side uploads through pinned staging: route table, layout, offsets
  size_t hbytes = 64 + 16 * (size_t)n_out + 8 * (size_t)n_out + 16 + blob + 16;
  if (up_scopes) hbytes += 20 * S + 64;
  if (up_res) hbytes += 12 * R + 64;
  if ((rc = b->emisc.need(hbytes))) return rc;
  uint8_t* h = b->emisc.p;
  size_t ho = up(64 + 16 * (size_t)n_out, 16);   // [0, 64): flags; then the totals
  auto upload = [&](void* dst, const void* src, size_t bytes) -> int {
    if (!bytes) return 0;
    std::memcpy(h + ho, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, h + ho, bytes, hipMemcpyHostToDevice, st));
    ho = up(ho + bytes, 16);
    return 0;
  };
  if (up_scopes && (b->lay.scope_span0.size() != S || b->lay.scope_hdr.size() != S || b->lay.scope_schema.size() != S))
    return 0;
  if (up_res && (b->lay.res_ref.size() != R || b->lay.res_scope0.size() != R)) return 0;
  if (blob && (rc = upload(routes, router->dev_blob.data(), blob))) return rc;
  if (up_scopes) {
    std::vector<uint32_t> s0(b->lay.scope_span0.begin(), b->lay.scope_span0.end());
    if ((rc = upload(scope_span0, s0.data(), 4 * S)) || (rc = upload(scope_hdr, b->lay.scope_hdr.data(), 8 * S)) ||
        (rc = upload(scope_schema, b->lay.scope_schema.data(), 8 * S)))
      return rc;
  }
  if (up_res &&
      ((rc = upload(res_ref, b->lay.res_ref.data(), 8 * R)) || (rc = upload(res_scope0, b->lay.res_scope0.data(), 4 * R))))
    return rc;
  a.pb = b->arena.p;
  a.n_spans = n;
  a.n_scopes = S;
  a.n_res = R;
  a.span_ref = b->d_spans;
  a.span_size = b->cols.span_size;
  a.keep = sampled ? outs->keep : nullptr;
  if (tmpl) {
    a.url_out = outs->url_out;
    a.tmpl = outs->tmpl;
    a.tmpl_arena = outs->tmpl_arena;
    a.tmpl_used = outs->tmpl_arena_used;
  }
  if (sql) a.sql_op = outs->sql_op;
  a.scope_span0 = up_scopes ? scope_span0 : b->d_span0;
  a.scope_hdr = up_scopes ? scope_hdr : b->d_hdr;
  a.scope_schema = up_scopes ? scope_schema : b->d_schema;
  a.scope_size = b->cols.scope_size;
  a.res_ref = up_res ? res_ref : b->d_res_ref;
  a.res_scope0 = up_res ? res_scope0 : b->d_res_scope0;
  a.res_size = b->cols.res_size;
  a.n_out = n_out;
  a.route_bits = router ? router->route_bits : 0;
  a.routes = reinterpret_cast<const EncRouteSlot*>(routes);
  a.route_keys = routes ? routes + router->dev_slots_bytes : nullptr;
  a.flags = reinterpret_cast<uint32_t*>(flags64);
  a.out_base = out_base;
  if ((n && !a.span_size) || (S && (!a.scope_span0 || !a.scope_hdr || !a.scope_schema || !a.scope_size)) ||
      (R && (!a.res_ref || !a.res_scope0 || !a.res_size)))
    return 0;
  using clk = std::chrono::steady_clock;
  auto t0 = clk::now();
  // sizing pass, offsets
  HIP_TRY(hipMemsetAsync(flags64, 0, 8, st));
  if (ca) {
    if ((uint64_t)ca_T * n) {
      HIP_TRY(hipMemcpyAsync(const_cast<uint8_t*>(ca_a.ca_src), ca->src, (size_t)ca_T * n, hipMemcpyDefault, st));
      HIP_TRY(hipMemcpyAsync(const_cast<ose_strref*>(ca_a.ca_val), ca->val, 8 * (size_t)ca_T * n, hipMemcpyDefault, st));
    }
    static_cast<EncArgs&>(ca_a) = a;
    ca_a.ca_blob = b->e->condattr_blob_dev;
    ca_a.ca_targets = ca_T;
    ca_a.ca_string_bytes = b->e->condattr_tab.string_bytes;
    ca_a.ca_arena_bytes = b->cols.arena_bytes;
    launch_enc_spans_ca(ca_a, st);
  } else {
    launch_enc_spans(a, st);
  }
  HIP_TRY(hipGetLastError());
  launch_enc_scopes(a, st);
  HIP_TRY(hipGetLastError());
  launch_enc_resources(a, st);
  HIP_TRY(hipGetLastError());
  launch_enc_scan(a, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h, flags64, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h + 64, a.out_total, 16 * (size_t)n_out, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint32_t fb;
  std::memcpy(&fb, h, 4);
  o->fallback = fb;
  o->t_ms[1] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  t0 = clk::now();
  if (fb) return 0;
  std::vector<uint64_t> tot(2 * (size_t)n_out);
  std::memcpy(tot.data(), h + 64, 16 * (size_t)n_out);
  std::vector<uint64_t> base(n_out);
  uint64_t all = 0;
  for (uint32_t k = 0; k < n_out; k++) {
    base[k] = all;
    all = up(all + tot[k], 16);
  }
  if ((rc = b->eout.need(all + 16))) return rc;
  a.out = b->eout.p;
  if ((rc = upload(out_base, base.data(), 8 * (size_t)n_out))) return rc;
  // host buffers (pinned, pooled with the workspace)
  o->outs.assign(n_out, EncodedOutput{});
  bool oom = false;
  for (uint32_t k = 0; k < n_out; k++) {
    EncodedOutput& x = o->outs[k];
    x.name = router ? (k + 1 < n_out ? router->pipelines[k] : std::string("default")) : std::string();
    x.len = tot[k];
    x.n_resources = (uint32_t)tot[n_out + k];
    x.data = encode_work_pinned(*o->work, x.len, &x.cap);
    x.pinned = true;
    oom |= x.data == nullptr;
  }
  if (oom) return fail(OSE_EDEVICE, "out of pinned host memory for the encoder outputs");
  o->t_ms[2] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  t0 = clk::now();
  if (ca) {
    static_cast<EncArgs&>(ca_a) = a;   // (a.out is set by now)
    launch_enc_write_ca(ca_a, st);
  } else {
    launch_enc_write(a, st);
  }
  HIP_TRY(hipGetLastError());
  for (uint32_t k = 0; k < n_out; k++)
    if (tot[k]) HIP_TRY(hipMemcpyAsync(o->outs[k].data, a.out + base[k], tot[k], hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h, flags64, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  std::memcpy(&fb, h, 4);
  if (fb & kEncFbWrite) return fail(OSE_EDEVICE, "GPU encoder: a record's bytes disagree with its size");
  if (res_off) {   // each output's offset of every resource's record (the scan the writer used)
    res_off->resize((size_t)n_out * R);
    if (R) HIP_TRY(hipMemcpy(res_off->data(), a.off, 8 * (size_t)n_out * R, hipMemcpyDeviceToHost));
  }
  o->t_ms[3] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  o->gpu = 1;
  *host = false;
  return 0;
}

int encode_threads() { return parallel_width(); }

// An OtlpOut with an encoder workspace from the engine's pool (a new one when
// the pool is empty); it holds an engine reference, dropped by
// otlp_out_release.  e NULL (the CPU test seams): no engine, a new workspace.
OtlpOut* checkout_out(Engine* e) {
  auto* o = new OtlpOut();
  o->e = e;
  if (e) {
    engine_retain(e);
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->enc_pool.empty()) {
      o->work = static_cast<EncodeWork*>(e->enc_pool.back());
      e->enc_pool.pop_back();
    }
  }
  if (!o->work) o->work = encode_work_new();
  return o;
}

// The GPU encoder first.  0 with *out set: it wrote the outputs; 0 with *out
// NULL: it declined the call and *fallback says why (the host encoder runs
// next); else an error code.
int encode_gpu_first(Engine* e, OtlpBatchImpl* b, const ose_outputs* outs, bool sampled, bool tmpl, bool sql,
                     const Router* router, hipStream_t st, OtlpOut** out, uint32_t* fallback,
                     std::vector<uint64_t>* res_off = nullptr, const ose_condattr_outputs* ca = nullptr) {
  *out = nullptr;
  OtlpOut* o = checkout_out(e);
  bool host = true;
  const int rc = encode_gpu(b, outs, sampled, tmpl, sql, router, st, o, &host, res_off, ca);
  if (rc || host) {
    *fallback = o->fallback;
    otlp_out_release(o);   // pinned buffers taken before a failure go back to the work's pool
    return rc;
  }
  *out = o;
  return 0;
}

// The host encoder on the message and its layout, with the decisions in host
// memory: the tail of every path that is not the GPU encoder's.  fallback: why
// the GPU encoder declined (0: not asked); t_start: when the call began (NULL
// for the seams, which report no D2H time); threads <= 0: the default width.
int finish_on_host(Engine* e, const uint8_t* pb, size_t len, const std::vector<uint64_t>& span_ref,
                   const OtlpLayout& lay, const EncodeDecisions& d, const ose_router* router, int threads,
                   uint32_t fallback, const std::chrono::steady_clock::time_point* t_start, ose_otlp_out** out) {
  OtlpOut* o = checkout_out(e);
  o->fallback = fallback;
  if (t_start)
    o->t_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - *t_start).count();
  std::string err;
  if (!encode_traces(pb, len, span_ref, lay, d, reinterpret_cast<const Router*>(router),
                     threads > 0 ? threads : encode_threads(), *o->work, o->outs, err, o->t_ms + 1)) {
    otlp_out_release(o);
    return fail(OSE_EINVAL, err);
  }
  *out = reinterpret_cast<ose_otlp_out*>(o);
  return 0;
}
}  // namespace

// The GPU encoder for the OTLP pipeline (otlp_pipeline.cpp): *out holds the
// batch's outputs and res_off every output's per-resource record offsets
// (n_out x R); *gpu false when the GPU encoder declined the batch (nothing
// in *out), the caller then takes its requests one by one.
int otlp_encode_gpu_offsets(Engine* e, ose_otlp_batch* bb, const ose_outputs* outs, uint32_t stages,
                            const Router* router, hipStream_t st, OtlpOut** out, std::vector<uint64_t>& res_off,
                            bool* gpu) {
  auto* b = reinterpret_cast<OtlpBatchImpl*>(bb);
  const bool sampled = stages & (OSE_STAGE_SAMPLE | OSE_STAGE_APPLY_KEEP);
  const bool tmpl = stages & OSE_STAGE_TEMPLATE;
  const bool sql = stages & (OSE_STAGE_SQLOP | OSE_STAGE_APPLY_SQLOP);
  uint32_t fallback = 0;
  const int rc = encode_gpu_first(e, b, outs, sampled, tmpl, sql, router, st, out, &fallback, &res_off);
  *gpu = *out != nullptr;
  return rc;
}

}  // namespace ose

using namespace ose;

extern "C" {

int ose_otlp_encode(ose_engine* eng, const ose_otlp_batch* bb, const ose_outputs* outs, uint32_t stages,
                    uint32_t group_mode, const ose_router* router, void* hip_stream, ose_otlp_out** out) {
  if (!eng || !bb || !out) return fail(OSE_EINVAL, "NULL argument");
  if (stages & OSE_STAGE_CONDATTR) return refuse_condattr("ose_otlp_encode");
  Engine* e = reinterpret_cast<Engine*>(eng);
  // odigossqldboperationprocessor's attribute and name are written only under
  // the engine option otlp_sqlop (the default until the next ABI version: refused)
  const bool sql = (stages & (OSE_STAGE_SQLOP | OSE_STAGE_APPLY_SQLOP)) != 0;
  if (sql && !(e->has_sqlop && e->option(Engine::kOptOtlpSqlop)))
    return fail(OSE_ENOTSUP, "ose_otlp_encode does not write odigossqldboperationprocessor's attribute and span name "
                             "(engine option otlp_sqlop is off)");
  if ((stages & OSE_STAGE_SQLOP) && (stages & OSE_STAGE_APPLY_SQLOP))
    return fail(OSE_EINVAL, "OSE_STAGE_APPLY_SQLOP and OSE_STAGE_SQLOP exclude each other");
  if (sql && (!outs || !outs->sql_op)) return fail(OSE_EINVAL, "sql_op is NULL");
  auto* b = const_cast<OtlpBatchImpl*>(reinterpret_cast<const OtlpBatchImpl*>(bb));
  if (b->e != e) return fail(OSE_EINVAL, "the batch belongs to another engine");
  if (int rc = bind_device(e)) return rc;
  const bool batch_mode = (stages & OSE_STAGE_SAMPLE) && group_mode == OSE_GROUP_BATCH;
  const bool sampled = (stages & (OSE_STAGE_SAMPLE | OSE_STAGE_APPLY_KEEP)) && !batch_mode;
  const bool tmpl = stages & OSE_STAGE_TEMPLATE;
  if ((sampled || batch_mode || tmpl) && !outs) return fail(OSE_EINVAL, "NULL outputs");
  if (sampled && !outs->keep) return fail(OSE_EINVAL, "keep is NULL");
  if (batch_mode && !outs->trace_keep) return fail(OSE_EINVAL, "trace_keep is NULL");
  if (tmpl && (!outs->url_out || !outs->tmpl || !outs->tmpl_arena || !outs->tmpl_arena_used))
    return fail(OSE_EINVAL, "template outputs are NULL");
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const auto t_start = std::chrono::steady_clock::now();
  const uint64_t n = b->cols.n_spans;
  uint32_t gpu_fallback = 0;
  if (!batch_mode) {   // the GPU encoder (OSE_GROUP_BATCH's all-or-nothing stays with the host)
    OtlpOut* o = nullptr;
    if (int rc = encode_gpu_first(e, b, outs, sampled, tmpl, sql, reinterpret_cast<const Router*>(router), st, &o,
                                  &gpu_fallback))
      return rc;
    if (o) {
      *out = reinterpret_cast<ose_otlp_out*>(o);
      return 0;
    }
  }
  // the decisions and the decoder's span sizes, D2H into the batch's pinned staging
  const size_t o_keep = 0, o_url = up(n + 16), o_tmpl = o_url + up(n + 16), o_size = o_tmpl + up(8 * n + 16),
               o_misc = o_size + up(4 * n + 16), o_sql = o_misc + 256, o_arena = o_sql + up(n + 16);
  // arena_used 0: the first pass, which brings tmpl_arena_used; else the pass
  // after the staging grew, which brings that many template bytes as well
  auto fetch = [&](uint8_t* h, uint64_t arena_used) -> int {
    if (n) HIP_TRY(hipMemcpyAsync(h + o_size, b->cols.span_size, 4 * n, hipMemcpyDeviceToHost, st));
    if (sampled && n) HIP_TRY(hipMemcpyAsync(h + o_keep, outs->keep, n, hipMemcpyDefault, st));
    if (batch_mode) HIP_TRY(hipMemcpyAsync(h + o_misc + 8, outs->trace_keep, 1, hipMemcpyDefault, st));
    if (sql && n) HIP_TRY(hipMemcpyAsync(h + o_sql, outs->sql_op, n, hipMemcpyDefault, st));
    if (tmpl) {
      if (n) HIP_TRY(hipMemcpyAsync(h + o_url, outs->url_out, n, hipMemcpyDefault, st));
      if (n) HIP_TRY(hipMemcpyAsync(h + o_tmpl, outs->tmpl, 8 * n, hipMemcpyDefault, st));
      if (!arena_used) HIP_TRY(hipMemcpyAsync(h + o_misc, outs->tmpl_arena_used, 8, hipMemcpyDefault, st));
      else HIP_TRY(hipMemcpyAsync(h + o_arena, outs->tmpl_arena, arena_used, hipMemcpyDefault, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  };
  int rc;
  if ((rc = b->stage.need(o_arena))) return rc;
  uint8_t* h = b->stage.p;
  if ((rc = fetch(h, 0))) return rc;
  uint64_t used = 0;
  if (tmpl) {
    std::memcpy(&used, h + o_misc, 8);
    if (used > outs->tmpl_arena_cap) return fail(OSE_ERANGE, "tmpl_arena_used beyond tmpl_arena_cap");
    if (used) {
      if ((rc = b->stage.need(o_arena + used))) return rc;   // grow-only: earlier contents are lost
      h = b->stage.p;
      if ((rc = fetch(h, used))) return rc;
    }
  }
  EncodeDecisions d;
  d.keep = sampled ? h + o_keep : nullptr;
  d.drop_all = batch_mode && !h[o_misc + 8];
  if (tmpl) {
    d.url_out = h + o_url;
    d.tmpl = reinterpret_cast<const ose_strref*>(h + o_tmpl);
    d.tmpl_arena = h + o_arena;
    d.tmpl_arena_len = used;
  }
  d.span_size = reinterpret_cast<const uint32_t*>(h + o_size);
  if (sql) d.sql_op = h + o_sql;
  if (b->released && !b->layout_on_host) {   // the released message buffer comes down once per release
    const size_t len = b->cols.arena_bytes;
    if ((rc = b->relhost.need(len + 16))) return rc;
    if (len) HIP_TRY(hipMemcpyAsync(b->relhost.p, b->arena.p, len, hipMemcpyDeviceToHost, st));
    b->pb = b->relhost.p;
    b->pb_len = len;
  }
  if ((rc = layout_to_host(b, st))) return rc;
  return finish_on_host(e, b->pb, b->pb_len, b->span_ref, b->lay, d, router, 0, gpu_fallback, &t_start, out);
}

int ose_otlp_encode_condattr(ose_engine* eng, const ose_otlp_batch* bb, const ose_condattr_outputs* ca,
                             const ose_router* router, void* hip_stream, ose_otlp_out** out) {
  if (!eng || !bb || !out) return fail(OSE_EINVAL, "NULL argument");
  Engine* e = reinterpret_cast<Engine*>(eng);
  if (!(e->has_condattr && e->option(Engine::kOptOtlpCondattr)))
    return fail(OSE_ENOTSUP, "ose_otlp_encode_condattr: the engine option otlp_condattr is off");
  auto* b = const_cast<OtlpBatchImpl*>(reinterpret_cast<const OtlpBatchImpl*>(bb));
  if (b->released) return fail(OSE_EINVAL, "ose_otlp_encode_condattr does not take a batch released by a groupbytrace store");
  if (b->e != e) return fail(OSE_EINVAL, "the batch belongs to another engine");
  if (!b->ca_on) return fail(OSE_EINVAL, "the batch was decoded with the engine option otlp_condattr off");
  const CondAttrCompiled& tab = e->condattr_tab;
  const uint64_t n = b->cols.n_spans;
  const uint32_t T = (uint32_t)tab.target_key.size();
  if (!ca || ((uint64_t)T * n && (!ca->src || !ca->val))) return fail(OSE_EINVAL, "src or val is NULL");
  if (int rc = bind_device(e)) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const auto t_start = std::chrono::steady_clock::now();
  uint32_t gpu_fallback = 0;
  {   // the GPU encoder
    OtlpOut* o = nullptr;
    if (int rc = encode_gpu_first(e, b, nullptr, false, false, false, reinterpret_cast<const Router*>(router), st, &o,
                                  &gpu_fallback, nullptr, ca))
      return rc;
    if (o) {
      *out = reinterpret_cast<ose_otlp_out*>(o);
      return 0;
    }
  }
  // the host encoder: the puts, the decoder's span sizes and what the decode
  // put behind the message bytes, D2H into the batch's pinned staging
  const uint64_t tail_base = std::min<uint64_t>(b->pb_len, b->cols.arena_bytes), tail = b->cols.arena_bytes - tail_base;
  const size_t o_src = 0, o_val = up((size_t)T * n + 16), o_size = o_val + up(8 * (size_t)T * n + 16),
               o_tail = o_size + up(4 * n + 16), o_end = o_tail + up(tail + 16);
  int rc;
  if ((rc = b->stage.need(o_end))) return rc;
  uint8_t* h = b->stage.p;
  if ((uint64_t)T * n) {
    HIP_TRY(hipMemcpyAsync(h + o_src, ca->src, (size_t)T * n, hipMemcpyDefault, st));
    HIP_TRY(hipMemcpyAsync(h + o_val, ca->val, 8 * (size_t)T * n, hipMemcpyDefault, st));
  }
  if (n) HIP_TRY(hipMemcpyAsync(h + o_size, b->cols.span_size, 4 * n, hipMemcpyDeviceToHost, st));
  if (tail) HIP_TRY(hipMemcpyAsync(h + o_tail, b->arena.p + tail_base, tail, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  std::string err;
  if ((rc = condattr_check_puts(h + o_src, reinterpret_cast<const ose_strref*>(h + o_val), n, T, b->cols.arena_bytes,
                                tab.string_bytes, err)))
    return fail(rc, err);
  std::vector<std::string> names(T);
  for (uint32_t u = 0; u < T; u++) names[u] = tab.keys[tab.target_key[u]];
  EncodeDecisions d;
  d.span_size = reinterpret_cast<const uint32_t*>(h + o_size);
  if ((uint64_t)T * n) {
    d.ca_src = h + o_src;
    d.ca_val = reinterpret_cast<const ose_strref*>(h + o_val);
    d.ca_targets = T;
    d.ca_names = names.data();
    d.ca_arena = b->pb;
    d.ca_tail_base = tail_base;
    d.ca_tail = h + o_tail;
    d.ca_strings = tab.blob.data() + tab.strings_off;
  }
  if ((rc = layout_to_host(b, st))) return rc;
  return finish_on_host(e, b->pb, b->pb_len, b->span_ref, b->lay, d, router, 0, gpu_fallback, &t_start, out);
}

// Test seam (CPU): the encoder on the host walk of `pb` with the given
// decisions (keep / url_out / tmpl NULL when absent) and span sizes
// computed on the host as the decoder would.  sql_op: OSE_SQLOP_* per span
// (odigossqldboperationprocessor's decisions), NULL when absent.
int osehost_otlp_encode_sql(const uint8_t* pb, size_t len, const uint8_t* keep, int drop_all, const uint8_t* url_out,
                            const ose_strref* tmpl, const uint8_t* tmpl_arena, uint64_t tmpl_arena_len,
                            const ose_router* router, int threads, ose_otlp_out** out, const uint8_t* sql_op) {
  if ((!pb && len) || !out) return fail(OSE_EINVAL, "NULL argument");
  std::vector<uint64_t> span_ref;
  OtlpLayout lay;
  std::vector<uint32_t> sizes;
  if (int rc = otlp_host_walk_sizes(pb, len, span_ref, lay, sizes)) return rc;
  EncodeDecisions d;
  d.keep = keep;
  d.drop_all = drop_all != 0;
  d.url_out = url_out;
  d.tmpl = tmpl;
  d.tmpl_arena = tmpl_arena;
  d.tmpl_arena_len = tmpl_arena_len;
  d.span_size = sizes.data();
  d.sql_op = sql_op;
  return finish_on_host(nullptr, pb, len, span_ref, lay, d, router, threads, 0, nullptr, out);
}

int osehost_otlp_encode(const uint8_t* pb, size_t len, const uint8_t* keep, int drop_all, const uint8_t* url_out,
                        const ose_strref* tmpl, const uint8_t* tmpl_arena, uint64_t tmpl_arena_len,
                        const ose_router* router, int threads, ose_otlp_out** out) {
  return osehost_otlp_encode_sql(pb, len, keep, drop_all, url_out, tmpl, tmpl_arena, tmpl_arena_len, router, threads, out,
                                 nullptr);
}

// Test seam (CPU): the host encoder applying odigosconditionalattributes' puts
// (what ose_otlp_encode_condattr's host path runs) on the host walk of `pb`.
// src / val: [n_targets * n_spans] as ose_condattr_outputs, host memory;
// arena: the bytes OSE_CA_ARENA values point into; strings: the string table
// of OSE_CA_CONFIG values; names: the target names' bytes back to back, their
// lengths in name_lens.  n_spans other than the message's is OSE_EINVAL; src
// and val are checked as ose_otlp_encode_condattr checks them.
int osehost_otlp_encode_condattr(const uint8_t* pb, size_t len, uint64_t n_spans, const uint8_t* src,
                                 const ose_strref* val, uint32_t n_targets, const uint8_t* arena, uint64_t arena_bytes,
                                 const uint8_t* strings, uint64_t string_bytes, const uint8_t* names,
                                 const uint32_t* name_lens, const ose_router* router, int threads, ose_otlp_out** out) {
  if ((!pb && len) || !out) return fail(OSE_EINVAL, "NULL argument");
  if (n_targets && n_spans && (!src || !val)) return fail(OSE_EINVAL, "src or val is NULL");
  if (n_targets && !name_lens) return fail(OSE_EINVAL, "NULL argument");
  std::vector<uint64_t> span_ref;
  OtlpLayout lay;
  std::vector<uint32_t> sizes;
  if (int rc = otlp_host_walk_sizes(pb, len, span_ref, lay, sizes)) return rc;
  if (span_ref.size() != n_spans) return fail(OSE_EINVAL, "n_spans is not the message's span count");
  std::string err;
  if (int rc = condattr_check_puts(src, val, n_spans, n_targets, arena_bytes, string_bytes, err)) return fail(rc, err);
  std::vector<std::string> target_names(n_targets);
  for (uint32_t u = 0, at = 0; u < n_targets; at += name_lens[u], u++)
    target_names[u].assign(reinterpret_cast<const char*>(names) + at, name_lens[u]);
  EncodeDecisions d;
  d.span_size = sizes.data();
  d.ca_src = src;
  d.ca_val = val;
  d.ca_targets = n_targets;
  d.ca_names = target_names.data();
  d.ca_arena = arena;
  d.ca_strings = strings;
  return finish_on_host(nullptr, pb, len, span_ref, lay, d, router, threads, 0, nullptr, out);
}

}  // extern "C"
