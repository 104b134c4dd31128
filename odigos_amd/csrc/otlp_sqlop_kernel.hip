// otlp_sqlop_kernel.hip — odigossqldboperationprocessor's span columns from
// the OTLP message (engine option otlp_sqlop).
//
// What the shim's columnising walk reads for the stage (columnize.cpp;
// odigossqldboperationprocessor/processor.go:52-64): Attributes().Get of
// "db.query.text" and of "db.operation.name", the first KeyValue of each key
// as pcommon.Map.Get finds it.
//
//   otlp_sqlop_kernel      one lane per span, after the span kernel
//                          (otlp_kernel.hip) on the same stream: the span's
//                          top-level fields, and of each attributes KeyValue
//                          the key and the value's place.  db_query is a ref
//                          into the message bytes (the arena): nothing is
//                          copied.  A db.query.text that is not a string_value
//                          needs AsString: the span joins the host pass's list.
//                          A span the span kernel listed is skipped.
//   otlp_sqlop_fix_kernel  the host pass's db_flags / db_query of the listed spans
//
// Every byte is read through ByteReader::at inside the span's payload, which
// the span kernel has walked already: the same 16-byte chunks, the same
// buffer contract (16 bytes of slack after the message).  No LDS; the one
// atomic is the host list's counter, as in the span kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_common.hpp"
#include "kernels.hpp"
#include "pb_device.hpp"

namespace ose {
namespace {
using namespace pbdev;

constexpr int kSqlThreads = 256;

constexpr uint64_t le(const char* s, int n) {
  uint64_t v = 0;
  for (int k = n - 1; k >= 0; k--) v = (v << 8) | (uint8_t)s[k];
  return v;
}
constexpr uint32_t kQueryLen = 13, kOpNameLen = 17;          // "db.query.text", "db.operation.name"
constexpr uint64_t kQuery0 = le("db.query", 8), kQuery1 = le(".text", 5);
constexpr uint64_t kOpName0 = le("db.opera", 8), kOpName1 = le("tion.nam", 8);

// bytes [o, o + n) of the message, little-endian (n <= 8)
__device__ __forceinline__ uint64_t load_le(Rd& r, uint32_t o, uint32_t n) {
  uint64_t v = 0;
  for (uint32_t k = 0; k < n; k++) v |= (uint64_t)r.br.at(o + k) << (8 * k);
  return v;
}

__global__ __launch_bounds__(kSqlThreads) void otlp_sqlop_kernel(OtlpSqlArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kSqlThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kSqlThreads + threadIdx.x; i < a.n_spans; i += stride) {
    if (a.host_flag[i]) continue;   // listed by the span kernel: the host pass writes both columns
    const uint64_t ref = a.span_ref[i];
    const uint32_t s0 = (uint32_t)ref, s1 = s0 + (uint32_t)(ref >> 32);
    Rd r(a.pb, s0, s1);
    uint32_t flags = 0;
    ose_strref query{0, 0};
    bool host = false;
    uint32_t f, wt;
    while (r.more() && r.tag(f, wt)) {
      uint32_t ps, pl;
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
      if (kl == kQueryLen && !(flags & OSE_DB_HAS_QUERY)) {
        if (load_le(r, ko, 8) != kQuery0 || load_le(r, ko + 8, 5) != kQuery1) continue;
        flags |= OSE_DB_HAS_QUERY;
        Val v{OSE_ATTR_OTHER, 0, 0, 0};
        if (has_val) any_value(r, vs, vs + vl, v);
        if (v.type == OSE_ATTR_STR) query = ose_strref{v.off, v.len};
        else host = true;   // AsString of an int, double, bool, bytes, array, kvlist or empty value
      } else if (kl == kOpNameLen && !(flags & OSE_DB_HAS_OPNAME)) {
        if (load_le(r, ko, 8) != kOpName0 || load_le(r, ko + 8, 8) != kOpName1 || r.br.at(ko + 16) != 'e') continue;
        flags |= OSE_DB_HAS_OPNAME;   // a value of any type
      }
    }
    if (r.bad || host) {
      a.host_flag[i] = 1;
      const uint32_t slot = atomicAdd(a.host_count, 1u);
      if (slot < a.host_cap) a.host_list[slot] = (uint32_t)i;
      continue;
    }
    a.db_flags[i] = (uint8_t)flags;
    a.db_query[i] = query;
  }
}

__global__ __launch_bounds__(kSqlThreads) void otlp_sqlop_fix_kernel(const OtlpSqlFix* fix, uint32_t n, uint8_t* db_flags,
                                                                     ose_strref* db_query) {
  const uint32_t q = blockIdx.x * kSqlThreads + threadIdx.x;
  if (q >= n) return;
  const OtlpSqlFix x = fix[q];
  db_flags[x.idx] = (uint8_t)x.flags;
  db_query[x.idx] = x.query;
}

}  // namespace

void launch_otlp_sqlop(const OtlpSqlArgs& a, hipStream_t st) {
  const uint64_t blocks = std::min<uint64_t>((a.n_spans + kSqlThreads - 1) / kSqlThreads, 16384);
  if (blocks) hipLaunchKernelGGL(otlp_sqlop_kernel, dim3((uint32_t)blocks), dim3(kSqlThreads), 0, st, a);
}

void launch_otlp_sqlop_fix(const OtlpSqlFix* fix, uint32_t n, uint8_t* db_flags, ose_strref* db_query, hipStream_t st) {
  const uint32_t blocks = (n + kSqlThreads - 1) / kSqlThreads;
  if (blocks) hipLaunchKernelGGL(otlp_sqlop_fix_kernel, dim3(blocks), dim3(kSqlThreads), 0, st, fix, n, db_flags, db_query);
}

}  // namespace ose
