// condattr_kernel.hip — odigosconditionalattributes on CDNA4 (gfx950).
//
// Replaces conditionalAttributesProcessor.processTraces
// (odigosconditionalattributes/processor.go:26-137).  The shim columnarises
// the attribute lookups per key (ose_condattr_columns) and applies PutStr
// from src / val.
//
//   condattr_scope_kernel  one lane per scope: everything that depends on the
//                          scope alone (condattr::scope_step): the action list
//                          a scope-name rule matches, the list a key rule
//                          gives a span without the key, and per target
//                          whether scope and resource both have the name.
//                          With the category-attributes profile the lookup
//                          among 269 scope names runs once per scope, not
//                          once per span.
//   condattr_span_kernel   one lane per span, grid-stride
//                          (condattr::span_step): hashes and compares the
//                          span's own value of a key rule through ByteReader
//                          (16-byte aligned arena loads, none leaves the
//                          allocation), runs the action lists, the defaults
//                          and span_size_out.
// The per-target state is the output columns (condattr_device.hpp).  No LDS,
// no atomics, no spins; plain vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "condattr_device.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace ose {
namespace {

constexpr int kCaThreads = 256;

struct DevEnv {
  using Reader = ByteReader;
  static __device__ __forceinline__ Reader reader(const uint8_t* p) { return ByteReader(p); }
};

__global__ __launch_bounds__(kCaThreads) void condattr_scope_kernel(CondAttrArgs a) {
  const condattr::View v = condattr::view(a.blob);
  const uint32_t s = blockIdx.x * kCaThreads + threadIdx.x;
  if (s < a.c.n_scopes) condattr::scope_step<DevEnv>(v, a.c, a.o.scratch, s);
}

__global__ __launch_bounds__(kCaThreads) void condattr_span_kernel(CondAttrArgs a) {
  const condattr::View v = condattr::view(a.blob);
  const uint64_t stride = (uint64_t)gridDim.x * kCaThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kCaThreads + threadIdx.x; i < a.c.n_spans; i += stride)
    condattr::span_step<DevEnv>(v, a.c, a.o, a.o.scratch, i);
}

}  // namespace

void launch_condattr_scopes(const CondAttrArgs& a, hipStream_t st) {
  const uint32_t blocks = (a.c.n_scopes + kCaThreads - 1) / kCaThreads;
  if (blocks) hipLaunchKernelGGL(condattr_scope_kernel, dim3(blocks), dim3(kCaThreads), 0, st, a);
}

void launch_condattr_spans(const CondAttrArgs& a, hipStream_t st) {
  constexpr uint64_t cap = 16384;
  const uint64_t blocks = std::min<uint64_t>((a.c.n_spans + kCaThreads - 1) / kCaThreads, cap);
  if (blocks) hipLaunchKernelGGL(condattr_span_kernel, dim3((uint32_t)blocks), dim3(kCaThreads), 0, st, a);
}

}  // namespace ose
