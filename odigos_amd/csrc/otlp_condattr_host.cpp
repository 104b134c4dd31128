// otlp_condattr_host.cpp — engine option otlp_condattr: odigosconditionalattributes'
// columns of a decoded OTLP batch (ose_otlp_condattr_columns).  otlp_host.cpp's
// decode() calls condattr_spans behind the span kernels and condattr_finish
// after the host pass.
#include <algorithm>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "columnize.hpp"
#include "otlp_batch.hpp"
#include "otlp_pb.hpp"
#include "taskpool.hpp"

namespace ose {

// The span columns on the GPU: the batch's slab of them, span_has zeroed,
// otlp_condattr_kernel behind the span kernel (before the host-pass count is
// read back: the kernel may add to the list).
int condattr_spans(Engine* e, OtlpBatchImpl* b, uint64_t n, const uint64_t* span_ref, const HostList& hl,
                   hipStream_t st) {
  const size_t K = e->condattr_tab.keys.size();
  const ose_columns& c = b->cols;
  const size_t N = std::max<uint64_t>(n, 1), S = std::max<uint32_t>(c.n_scopes, 1), R = std::max<uint32_t>(c.n_resources, 1);
  ose_condattr_columns& ca = b->ca;
  ca = ose_condattr_columns{};
  const std::vector<SlabPart> parts = {
      {(void**)&ca.span_has, K * N}, {(void**)&ca.span_val, 8 * K * N}, {(void**)&ca.span_kv_size, 4 * K * N},
      {(void**)&ca.scope_name, 8 * S}, {(void**)&ca.scope_has, K * S}, {(void**)&ca.scope_val, 8 * K * S},
      {(void**)&ca.res_has, K * R}, {(void**)&ca.res_val, 8 * K * R},
  };
  if (int rc = slab_place(b->caslab, parts)) return rc;
  b->ca_keys = (uint32_t)K;
  if (!n || !K) return 0;
  HIP_TRY(hipMemsetAsync(const_cast<uint8_t*>(ca.span_has), 0, K * N, st));
  OtlpCondAttrArgs a{};
  a.pb = b->arena.p;
  a.n_spans = n;
  a.span_ref = span_ref;
  a.blob = e->condattr_blob_dev;
  a.slots = static_cast<const OtlpCaSlot*>(e->condattr_slots_dev);
  a.slot_mask = e->condattr_slot_mask;
  a.key_lens = e->condattr_key_lens;
  a.span_has = const_cast<uint8_t*>(ca.span_has);
  a.span_val = const_cast<ose_strref*>(ca.span_val);
  a.span_kv_size = const_cast<uint32_t*>(ca.span_kv_size);
  set_host_list(a, hl);
  return e->timed("otlp_condattr_kernel", st, [&] { launch_otlp_condattr(a, st); });
}

// The rest, after the host pass: the K entries of every listed span (pb_span
// and the columniser's lookup, written by otlp_condattr_fix_kernel), and the
// per-scope and per-resource columns, made on the host from the message bytes
// at the scopes' InstrumentationScope refs and the resources' Resource fields
// (S and R are small against N; equal header bytes are looked up once).  The
// strings go after the arena's bytes (the message, then the host pass's
// strings); the arena is regrown when they do not fit.
int condattr_finish(Engine* e, OtlpBatchImpl* b, const uint8_t* pb, const std::vector<uint32_t>& list,
                    const uint32_t* host_list, hipStream_t st) {
  const std::vector<std::string>& keys = e->condattr_tab.keys;
  const size_t K = keys.size();
  ose_columns& c = b->cols;
  const uint64_t n = c.n_spans, S = c.n_scopes, R = c.n_resources;
  const size_t cnt = list.size();
  // the scopes' and resources' refs: on the host already, or fetched (these
  // three arrays only: the span refs stay on the device)
  std::vector<uint64_t> hdr_d, sref_d, rref_d;
  const uint64_t *hdr = b->lay.scope_hdr.data(), *sref = b->lay.scope_ref.data(), *rref = b->lay.res_ref.data();
  if (!b->layout_on_host) {
    hdr_d.resize(S);
    if (S) HIP_TRY(hipMemcpyAsync(hdr_d.data(), b->d_hdr, 8 * S, hipMemcpyDeviceToHost, st));
    hdr = hdr_d.data();
    if (b->res_on_device) {
      sref_d.resize(S);
      rref_d.resize(R);
      if (S) HIP_TRY(hipMemcpyAsync(sref_d.data(), b->d_scope_ref, 8 * S, hipMemcpyDeviceToHost, st));
      if (R) HIP_TRY(hipMemcpyAsync(rref_d.data(), b->d_res_ref, 8 * R, hipMemcpyDeviceToHost, st));
      sref = sref_d.data();
      rref = rref_d.data();
    }
    HIP_TRY(hipStreamSynchronize(st));
  }
  // behind the host pass's strings, or, without any, behind the message's 16
  // zero bytes of slack, where the host pass's would start
  const size_t base = std::max<size_t>(c.arena_bytes, up(b->pb_len + 16, 16));
  std::string strs;
  ProtoSizer sizer;
  auto pad = [](size_t x) { return std::max<size_t>(x, 1); };
  std::vector<uint8_t> fix_has(pad(K * cnt), 0), scope_has(pad(K * S), 0), res_has(pad(K * R), 0);
  std::vector<ose_strref> fix_val(pad(K * cnt), ose_strref{0, 0}), scope_val(pad(K * S), ose_strref{0, 0}),
      res_val(pad(K * R), ose_strref{0, 0}), scope_name(pad(S), ose_strref{0, 0});
  std::vector<uint32_t> fix_kv(pad(K * cnt), 0);
  for (size_t q = 0; q < cnt; q++) {
    const uint64_t ref = b->span_ref[list[q]];   // (the host pass brought the layout back)
    Span sp;
    if (!pb_span(pb + (uint32_t)ref, (size_t)(ref >> 32), sp)) return fail(OSE_EINVAL, "OTLP protobuf: malformed Span");
    condattr_lookup(keys, sp.attrs, q, cnt, strs, base, sizer, fix_has.data(), fix_val.data(), fix_kv.data());
  }
  auto copy_row = [&](std::vector<uint8_t>& has, std::vector<ose_strref>& val, size_t rows, size_t from, size_t to) {
    for (size_t k = 0; k < K; k++) {
      has[k * rows + to] = has[k * rows + from];
      val[k * rows + to] = val[k * rows + from];
    }
  };
  // The scopes and the resources, split over threads (a node's batch may hold
  // a scope for every few spans): each thread looks equal header bytes up once,
  // collects its strings with refs relative to them, and the refs are moved to
  // the strings' final place once every thread's share is known.
  const int T = (int)std::min<uint64_t>((uint64_t)std::max(1, parallel_width()), std::max<uint64_t>(1, (S + R) / 4096));
  struct Share { std::string strs, err; };
  std::vector<Share> share((size_t)T);
  auto scopes_of = [&](Share& me, size_t s_lo, size_t s_hi) {
    std::unordered_map<std::string_view, size_t> seen;
    for (size_t s = s_lo; s < s_hi; s++) {
      const uint64_t h = hdr[s];
      ScopeSpans meta;
      if (h != OtlpLayout::kMulti) {
        const std::string_view key((const char*)pb + (uint32_t)h, (size_t)(h >> 32));
        auto it = seen.find(key);
        if (it != seen.end()) {
          scope_name[s] = scope_name[it->second];
          copy_row(scope_has, scope_val, S, it->second, s);
          continue;
        }
        seen.emplace(key, s);
        if (!pb_scope(pb + (uint32_t)h, (size_t)(h >> 32), meta)) { me.err = "OTLP protobuf: malformed InstrumentationScope"; return; }
      } else {   // several scope fields: merged, as the encoder's scope_header does
        const uint64_t sr = sref[s];
        PbReader r(pb + (uint32_t)sr, (size_t)(sr >> 32));
        uint32_t f, wt;
        while (r.more() && r.tag(f, wt)) {
          size_t o, l;
          if (f == 1 && wt == 2 && r.bytes(o, l)) {
            if (!pb_scope(pb + (uint32_t)sr + o, l, meta)) { me.err = "OTLP protobuf: malformed InstrumentationScope"; return; }
          } else if (f != 1) {
            r.skip(wt, f);
          } else {
            r.fail();
          }
        }
        if (!r.ok) { me.err = "OTLP protobuf: malformed ScopeSpans"; return; }
      }
      scope_name[s] = ose_strref{(uint32_t)me.strs.size(), (uint32_t)meta.scope_name.size()};
      me.strs += meta.scope_name;
      condattr_lookup(keys, meta.scope_attrs, s, S, me.strs, 0, sizer, scope_has.data(), scope_val.data(), nullptr);
    }
  };
  auto resources_of = [&](Share& me, size_t r_lo, size_t r_hi) {
    std::unordered_map<std::string_view, size_t> seen;
    std::vector<std::pair<size_t, size_t>> rf;   // the Resource fields (merged when several)
    for (size_t ri = r_lo; ri < r_hi; ri++) {
      const size_t ro = (uint32_t)rref[ri], rl = (size_t)(rref[ri] >> 32);
      PbReader p(pb + ro, rl);
      rf.clear();
      uint32_t f, wt;
      while (p.more() && p.tag(f, wt)) {
        size_t o, l;
        if (wt == 2 && f == 1) {
          if (!p.bytes(o, l)) break;
          rf.emplace_back(ro + o, l);
        } else {
          p.skip(wt, f);
        }
      }
      if (!p.ok) { me.err = "OTLP protobuf: malformed ResourceSpans"; return; }
      if (rf.size() == 1) {
        const std::string_view key((const char*)pb + rf[0].first, rf[0].second);
        auto it = seen.find(key);
        if (it != seen.end()) {
          copy_row(res_has, res_val, R, it->second, ri);
          continue;
        }
        seen.emplace(key, ri);
      }
      AttrMap attrs;
      uint32_t dropped = 0;
      for (auto& x : rf)
        if (!pb_resource(pb + x.first, x.second, attrs, dropped)) { me.err = "OTLP protobuf: malformed Resource"; return; }
      condattr_lookup(keys, attrs, ri, R, me.strs, 0, sizer, res_has.data(), res_val.data(), nullptr);
    }
  };
  parallel_run(T, [&](int t) {
    scopes_of(share[(size_t)t], S * t / T, S * (t + 1) / T);
    if (share[(size_t)t].err.empty()) resources_of(share[(size_t)t], R * t / T, R * (t + 1) / T);
  });
  for (auto& sh : share)
    if (!sh.err.empty()) return fail(OSE_EINVAL, sh.err);
  std::vector<size_t> share_at((size_t)T);
  {
    size_t at = base + strs.size();
    for (int t = 0; t < T; t++) {
      share_at[(size_t)t] = at;
      at += share[(size_t)t].strs.size();
    }
    if (at > 0xFFFFFFF0ull) return fail(OSE_ERANGE, "OTLP ingest: the arena passes 4 GiB");
  }
  parallel_run(T, [&](int t) {
    const uint32_t add = (uint32_t)share_at[(size_t)t];
    for (size_t s = S * t / T; s < S * (t + 1) / T; s++) {
      scope_name[s].off += add;
      for (size_t k = 0; k < K; k++)
        if (scope_has[k * S + s]) scope_val[k * S + s].off += add;
    }
    for (size_t ri = R * t / T; ri < R * (t + 1) / T; ri++)
      for (size_t k = 0; k < K; k++)
        if (res_has[k * R + ri]) res_val[k * R + ri].off += add;
  });
  for (auto& sh : share) strs += sh.strs;
  const size_t end = base + strs.size();
  if (end > 0xFFFFFFF0ull) return fail(OSE_ERANGE, "OTLP ingest: the arena passes 4 GiB");
  int rc;
  if ((rc = regrow_arena(b, base, end + 16, st))) return rc;   // what the arena holds moves with it
  ose_condattr_columns& ca = b->ca;
  auto upl = [&](const void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
  };
  HIP_TRY(upl(b->arena.p + base, strs.data(), strs.size()));
  HIP_TRY(upl(ca.scope_name, scope_name.data(), 8 * S));
  HIP_TRY(upl(ca.scope_has, scope_has.data(), K * S));
  HIP_TRY(upl(ca.scope_val, scope_val.data(), 8 * K * S));
  HIP_TRY(upl(ca.res_has, res_has.data(), K * R));
  HIP_TRY(upl(ca.res_val, res_val.data(), 8 * K * R));
  if (cnt && K) {
    const size_t hb = up(K * cnt + 16), vb = up(8 * K * cnt + 16), kb = up(4 * K * cnt + 16);
    if ((rc = b->cafix.need(hb + vb + kb))) return rc;
    HIP_TRY(upl(b->cafix.p, fix_has.data(), K * cnt));
    HIP_TRY(upl(b->cafix.p + hb, fix_val.data(), 8 * K * cnt));
    HIP_TRY(upl(b->cafix.p + hb + vb, fix_kv.data(), 4 * K * cnt));
    OtlpCondAttrFixArgs fa{};
    fa.cnt = (uint32_t)cnt;
    fa.n_keys = (uint32_t)K;
    fa.n_spans = n;
    fa.list = host_list;
    fa.fix_has = b->cafix.p;
    fa.fix_val = reinterpret_cast<const ose_strref*>(b->cafix.p + hb);
    fa.fix_kv = reinterpret_cast<const uint32_t*>(b->cafix.p + hb + vb);
    fa.span_has = const_cast<uint8_t*>(ca.span_has);
    fa.span_val = const_cast<ose_strref*>(ca.span_val);
    fa.span_kv_size = const_cast<uint32_t*>(ca.span_kv_size);
    launch_otlp_condattr_fix(fa, st);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));   // the sources are on this stack
  c.arena_bytes = end;
  ca.n_spans = n;
  ca.n_resources = (uint32_t)R;
  ca.n_scopes = (uint32_t)S;
  ca.arena_bytes = end;
  ca.arena = c.arena;
  ca.scope = c.scope;
  ca.scope_resource = c.scope_resource;
  ca.span_size = c.span_size;
  b->ca_on = true;
  return 0;
}

}  // namespace ose
