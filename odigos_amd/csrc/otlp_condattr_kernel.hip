// otlp_condattr_kernel.hip — odigosconditionalattributes' span columns from
// the OTLP message (engine option otlp_condattr).
//
// What the shim's columnising walk reads for the stage (columnize.cpp
// columnize_condattr; odigosconditionalattributes/processor.go:68, :80, :88):
// Attributes().Get of every key of the compiled config, the first KeyValue of
// each key as pcommon.Map.Get finds it.
//
//   otlp_condattr_kernel      one lane per span, after the span kernel
//                             (otlp_kernel.hip) on the same stream: the span's
//                             top-level fields, and of each attributes KeyValue
//                             the key and the value's place.  The key is looked
//                             up among the engine's keys: its length against a
//                             mask of the lengths there are, then its FNV-1a in
//                             an open-addressing table (OtlpCaSlot), then the
//                             bytes.  A hit stores span_has = 1, span_val (a
//                             ref into the message bytes: nothing is copied)
//                             and, for a target key, span_kv_size.  A matched
//                             key whose value is not a string_value needs
//                             AsString: the span joins the host pass's list.  A
//                             span the span kernel listed is skipped.
//   otlp_condattr_fix_kernel  the host pass's K entries of every listed span
//
// span_has is zeroed before the launch and a lane reads back only its own
// stores (has this key been seen in this span), so no per-lane state is
// indexed by a key number and the number of keys is unbounded.  Every message
// byte is read through ByteReader::at inside the span's payload, which the
// span kernel has walked already: the same 16-byte chunks, the same buffer
// contract (16 bytes of slack after the message).  No LDS; the one atomic is
// the host list's counter, as in the span kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "condattr_device.hpp"
#include "device_common.hpp"
#include "kernels.hpp"
#include "pb_device.hpp"

namespace ose {
namespace {
using namespace pbdev;

constexpr int kCaThreads = 256;

__global__ __launch_bounds__(kCaThreads) void otlp_condattr_kernel(OtlpCondAttrArgs a) {
  const condattr::View v = condattr::view(a.blob);
  const uint64_t n = a.n_spans;
  const uint64_t stride = (uint64_t)gridDim.x * kCaThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kCaThreads + threadIdx.x; i < n; i += stride) {
    if (a.host_flag[i]) continue;   // listed by the span kernel: the host pass writes every entry
    const uint64_t ref = a.span_ref[i];
    const uint32_t s0 = (uint32_t)ref, s1 = s0 + (uint32_t)(ref >> 32);
    Rd r(a.pb, s0, s1);
    bool host = false;
    while (r.more()) {
      uint32_t f, wt, ps, pl;
      if (!r.tag(f, wt)) break;
      if (f != 9 || wt != 2) { r.skip(wt); continue; }
      if (!r.len(ps, pl)) break;
      // the KeyValue: key (1) and value (2); the span kernel sent a span
      // with either field repeated to the host pass
      const uint32_t save_i = r.i, save_end = r.end;
      r.i = ps;
      r.end = ps + pl;
      uint32_t ko = 0, kl = 0, vs = 0, vl = 0, f2, w2;
      bool has_val = false;
      while (r.more() && r.tag(f2, w2)) {
        uint32_t qs, ql;
        if ((f2 == 1 || f2 == 2) && w2 == 2) {
          if (!r.len(qs, ql)) break;
          if (f2 == 1) { ko = qs; kl = ql; }
          else { vs = qs; vl = ql; has_val = true; }
        } else {
          r.skip(w2);
        }
      }
      r.i = save_i;
      r.end = save_end;
      if (r.bad) break;
      if (!((a.key_lens >> (kl < 63 ? kl : 63)) & 1)) continue;   // no key of this length
      uint32_t h = 2166136261u;
      for (uint32_t q = 0; q < kl; q++) h = (h ^ r.br.at(ko + q)) * 16777619u;
      uint32_t k = condattr::kNone;
      uint32_t p = h & a.slot_mask;
      for (uint32_t step = 0; step <= a.slot_mask; step++, p = (p + 1) & a.slot_mask) {
        const OtlpCaSlot sl = a.slots[p];
        if (sl.key == condattr::kNone) break;
        if (sl.hash != h) continue;
        const condattr::Key key = v.keys[sl.key];
        if (key.len != kl) continue;
        const uint8_t* kb = v.strings + key.off;
        uint32_t q = 0;
        while (q < kl && r.br.at(ko + q) == kb[q]) q++;
        if (q == kl) { k = sl.key; break; }
      }
      if (k == condattr::kNone) continue;
      if (a.span_has[k * n + i]) continue;   // Map.Get: the first KeyValue of the key
      Val val{OSE_ATTR_OTHER, 0, 0, 0};
      if (has_val) any_value(r, vs, vs + vl, val);
      if (r.bad || val.type != OSE_ATTR_STR) {   // AsString of an int, double, bool, bytes, array, kvlist or empty value
        host = true;
        break;
      }
      a.span_has[k * n + i] = 1;
      a.span_val[k * n + i] = ose_strref{val.off, val.len};
      if (v.keys[k].target != condattr::kNone)
        a.span_kv_size[k * n + i] = (uint32_t)field_len(str_field(kl) + field_len(field_len(val.len)));
    }
    if (r.bad || host) {
      a.host_flag[i] = 1;
      const uint32_t slot = atomicAdd(a.host_count, 1u);
      if (slot < a.host_cap) a.host_list[slot] = (uint32_t)i;
    }
  }
}

__global__ __launch_bounds__(kCaThreads) void otlp_condattr_fix_kernel(OtlpCondAttrFixArgs a) {
  const uint64_t x = (uint64_t)blockIdx.x * kCaThreads + threadIdx.x;
  if (x >= (uint64_t)a.cnt * a.n_keys) return;
  const uint64_t k = x / a.cnt, q = x % a.cnt;   // key-major, as the columns
  const uint64_t at = k * a.n_spans + a.list[q];
  a.span_has[at] = a.fix_has[x];
  a.span_val[at] = a.fix_val[x];
  a.span_kv_size[at] = a.fix_kv[x];
}

}  // namespace

void launch_otlp_condattr(const OtlpCondAttrArgs& a, hipStream_t st) {
  const uint64_t blocks = std::min<uint64_t>((a.n_spans + kCaThreads - 1) / kCaThreads, 16384);
  if (blocks) hipLaunchKernelGGL(otlp_condattr_kernel, dim3((uint32_t)blocks), dim3(kCaThreads), 0, st, a);
}

void launch_otlp_condattr_fix(const OtlpCondAttrFixArgs& a, hipStream_t st) {
  const uint64_t blocks = ((uint64_t)a.cnt * a.n_keys + kCaThreads - 1) / kCaThreads;
  if (blocks) hipLaunchKernelGGL(otlp_condattr_fix_kernel, dim3((uint32_t)blocks), dim3(kCaThreads), 0, st, a);
}

}  // namespace ose
