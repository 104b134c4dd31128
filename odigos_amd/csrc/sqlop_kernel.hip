// sqlop_kernel.hip — odigossqldboperationprocessor on CDNA4 (gfx950).
//
// Replaces DBOperationProcessor.processTraces (odigossqldboperationprocessor/
// processor.go:30-78): per span with db.query.text and without
// db.operation.name, in a resource shouldExcludeLanguage (:119-143) lets
// through, the operation DetectSQLOperationName (:84-115) finds in the query.
// The shim columnarises the attribute lookups (db_flags, db_query,
// res_sql_ok) and applies PutStr / SetName from sql_op.
//
//   sqlop_kernel            one lane per span; the first 16 bytes of the
//                           query decide in registers when they hold the
//                           leading ASCII blanks, the keyword and its
//                           terminator; everything else (non-ASCII spaces,
//                           U+017F / U+0131 letters, long blank runs, a word
//                           ended by \r \v \f) walks the bytes through
//                           ByteReader with the classifier of sqlop_device.hpp
//   sqlop_size_span_kernel  the spans pass of odigostrafficmetrics after this
//                           stage: size_span_kernel (size_kernel.hip) plus the
//                           attribute and the longer name of the spans with
//                           sql_op != 0
// No LDS in sqlop_kernel, no atomics, no spins; plain vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_common.hpp"
#include "kernels.hpp"
#include "size_device.hpp"
#include "sqlop_device.hpp"

namespace ose {
namespace {

constexpr int kQThreads = 256;
constexpr uint32_t kGeneral = 0xFFu;   // the window does not decide

constexpr uint64_t le(const char* s, int n) {
  uint64_t v = 0;
  for (int k = n - 1; k >= 0; k--) v = (v << 8) | (uint8_t)s[k];
  return v;
}

// The first min(len, 16) bytes of the string at s as two little-endian
// words, bytes past the string zeroed: one aligned 16-byte load, a second
// only when those bytes cross into the next chunk (that chunk then holds a
// byte of the string, so the load stays inside the arena's allocation).
__device__ __forceinline__ void load_window(const uint8_t* s, uint32_t m, uint64_t& A, uint64_t& B) {
  const uint64_t addr = (uint64_t)s;
  const uint32_t o = (uint32_t)(addr & 15);
  const uint4* al = reinterpret_cast<const uint4*>(addr & ~15ull);
  const uint4 a = al[0];
  uint4 b = make_uint4(0, 0, 0, 0);
  if (o + m > 16) b = al[1];
  // shift the eight words right by o bytes: 8, 4, then o & 3 (selects on
  // named registers: a runtime word index would go to scratch)
  uint32_t w0 = a.x, w1 = a.y, w2 = a.z, w3 = a.w, w4 = b.x, w5 = b.y, w6 = b.z, w7 = b.w;
  if (o & 8) w0 = w2, w1 = w3, w2 = w4, w3 = w5, w4 = w6, w5 = w7;
  if (o & 4) w0 = w1, w1 = w2, w2 = w3, w3 = w4, w4 = w5;
  const uint32_t sh = o & 3;
  const uint32_t x0 = __builtin_amdgcn_alignbyte(w1, w0, sh), x1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
  const uint32_t x2 = __builtin_amdgcn_alignbyte(w3, w2, sh), x3 = __builtin_amdgcn_alignbyte(w4, w3, sh);
  A = x0 | ((uint64_t)x1 << 32);
  B = x2 | ((uint64_t)x3 << 32);
  if (m < 8) A &= (1ull << (8 * m)) - 1;
  if (m <= 8) B = 0;
  else if (m < 16) B &= (1ull << (8 * (m - 8))) - 1;
}

// The decision from the window, or kGeneral.  It decides only on ASCII: a
// byte >= 0x80 among the seven bytes from the first non-blank one sends the
// span to the general path.
__device__ __forceinline__ uint32_t window_detect(uint64_t A, uint64_t B, uint32_t m, uint32_t len) {
  uint32_t k = 0;
  for (; k < m; k++) {
    const uint32_t b = (uint32_t)((k < 8 ? A >> (8 * k) : B >> (8 * (k - 8))) & 0xFFu);
    if (!sqlop::ascii_space(b)) break;
  }
  if (k == m) return m == len ? sqlop::kNone : kGeneral;   // blanks only: UNKNOWN when that is the whole query
  uint64_t v;
  if (k == 0) v = A;
  else if (k < 8) v = (A >> (8 * k)) | (B << (64 - 8 * k));
  else v = B >> (8 * (k - 8));
  const uint32_t avail = m - k;   // bytes of v inside the string and the window (the rest are zero)
  if (v & 0x0080808080808080ull) return kGeneral;
  const uint64_t u = v & 0xDFDFDFDFDFDFDFDFull;   // (b & 0xDF) == 'K' only for b in {'K', 'k'}
  const uint64_t u6 = u & 0xFFFFFFFFFFFFull;
  uint32_t op = sqlop::kNone, L = 6;
  if (u6 == le("SELECT", 6)) op = sqlop::kSelect;
  else if (u6 == le("INSERT", 6)) op = sqlop::kInsert;
  else if (u6 == le("UPDATE", 6)) op = sqlop::kUpdate;
  else if (u6 == le("DELETE", 6)) op = sqlop::kDelete;
  else if (u6 == le("CREATE", 6)) op = sqlop::kCreate;
  else if ((u & 0xFFFFFFFFFFull) == le("ALTER", 5)) op = sqlop::kAlter, L = 5;
  else if ((u & 0xFFFFFFFFull) == le("DROP", 4)) op = sqlop::kDrop, L = 4;
  const bool whole = m == len;   // the window holds the query's end
  if (!op) return (avail >= 6 || whole) ? sqlop::kNone : kGeneral;
  if (avail == L) return whole ? op : kGeneral;
  const uint32_t t = (uint32_t)((v >> (8 * L)) & 0xFFu);   // < 0x80 (checked above)
  if (sqlop::delimiter(t)) return op;
  return sqlop::ascii_space(t) ? kGeneral : sqlop::kNone;   // \r \v \f: the rest must be spaces only
}

__global__ __launch_bounds__(kQThreads) void sqlop_kernel(SqlOpArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kQThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kQThreads + threadIdx.x; i < a.n_spans; i += stride) {
    // every column up front: one memory round trip before the arena's
    const uint32_t f = a.db_flags[i];
    const ose_strref q = a.db_query[i];
    uint32_t ok = 1;
    if (a.res_sql_ok) ok = a.res_sql_ok[a.resource[i]];
    uint32_t op = sqlop::kNone;
    // processor.go:52-61: db.query.text found, db.operation.name not
    if (ok && (f & (OSE_DB_HAS_QUERY | OSE_DB_HAS_OPNAME)) == OSE_DB_HAS_QUERY && q.len) {
      const uint8_t* s = a.arena + q.off;
      const uint32_t m = q.len < 16u ? q.len : 16u;
      uint64_t A, B;
      load_window(s, m, A, B);
      op = window_detect(A, B, m, q.len);
      if (op == kGeneral) {
        ByteReader rd(s);
        op = sqlop::detect(rd, q.len);
      }
    }
    a.sql_op[i] = (uint8_t)op;
  }
}

using namespace sizedev;

// strlen(NAME[op]) of processor.go:19-27
__device__ __forceinline__ uint32_t op_len(uint32_t op) { return op == OSE_SQLOP_DROP ? 4u : op == OSE_SQLOP_ALTER ? 5u : 6u; }

// size_span_load's columns plus what SQLOP adds to a surviving span:
// PutStr("db.operation.name", NAME) is one more KeyValue (key 17 bytes) and
// SetName(name + " " + NAME) reframes the name, whose length here is what the
// URL stage left (method + " " + template after a rename).
__device__ __forceinline__ SpanCols sql_span_load(const SqlSizeArgs& a, uint64_t i) {
  SpanCols x = size_span_load(a.sz, i);
  if (x.valid) {
    const uint32_t op = a.sql_op[i];
    const uint32_t nl = a.sz.templated ? x.old : a.sz.name_len[i];
    if (op && x.kept) {
      const uint64_t ol = op_len(op);
      const uint64_t L = (x.u & OSE_OUT_RENAME) ? (uint64_t)nl + 1 + x.tl : nl;
      const uint64_t add = field_len(field_len(17) + field_len(field_len(ol))) + field_len(L + 1 + ol) - (L ? field_len(L) : 0);
      x.span_size += (uint32_t)add;
    }
  }
  return x;
}

// size_span_kernel's walk (size_kernel.hip): grid-stride over 256-span tiles,
// two tiles in flight, the surviving-span count added once per block.
__global__ __launch_bounds__(kQThreads) void sqlop_size_span_kernel(SqlSizeArgs a) {
  if (size_batch_dropped(a.sz)) return;
  __shared__ uint32_t wk[kQThreads / kWave];
  uint32_t kept_total = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kQThreads;
  for (uint64_t base = (uint64_t)blockIdx.x * kQThreads; base < a.sz.n_spans; base += 2 * stride) {
    const SpanCols x0 = sql_span_load(a, base + threadIdx.x);
    const SpanCols x1 = sql_span_load(a, base + stride + threadIdx.x);
    kept_total += size_span_finish(a.sz, x0);
    if (base + stride < a.sz.n_spans) kept_total += size_span_finish(a.sz, x1);   // wave-uniform
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kept_total += __shfl_xor(kept_total, o, kWave);
  if ((threadIdx.x & 63) == 0) wk[threadIdx.x >> 6] = kept_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t k = 0;
    for (int w = 0; w < kQThreads / kWave; w++) k += wk[w];
    if (k) atomicAdd((unsigned long long*)a.sz.accepted, (unsigned long long)k);
  }
}

}  // namespace

void launch_sqlop(const SqlOpArgs& a, hipStream_t st) {
  constexpr uint64_t cap = 16384;
  const uint64_t blocks = std::min<uint64_t>((a.n_spans + kQThreads - 1) / kQThreads, cap);
  if (blocks) hipLaunchKernelGGL(sqlop_kernel, dim3((uint32_t)blocks), dim3(kQThreads), 0, st, a);
}

void launch_sqlop_size_spans(const SqlSizeArgs& a, hipStream_t st) {
  constexpr uint64_t cap = 1024;   // launch_size_spans' grid
  const uint64_t blocks = std::min<uint64_t>((a.sz.n_spans + kQThreads - 1) / kQThreads, cap);
  if (blocks) hipLaunchKernelGGL(sqlop_size_span_kernel, dim3((uint32_t)blocks), dim3(kQThreads), 0, st, a);
}

}  // namespace ose
