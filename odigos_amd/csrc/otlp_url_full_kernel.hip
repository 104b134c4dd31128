// otlp_url_full_kernel.hip — the Path of net/url.Parse(url.full | http.url)
// from the OTLP message (engine option otlp_url_full).
//
// What the shim's columnising walk does for a span with a method and neither
// url.path nor http.target (columnize.cpp; odigosurltemplateprocessor/
// processor.go:196-208): the first url.full KeyValue, else the first
// http.url, AsString, url.Parse, and on success the Path as the span's path.
//
//   otlp_url_full_kernel           one lane per span, after the span kernel
//                                  (otlp_kernel.hip) on the same stream, for
//                                  the spans it finished with HAS_METHOD and
//                                  PATH_NONE.  url_full.hpp's parser runs over
//                                  the value's bytes where they are.  A Path
//                                  without escapes is a ref into the message
//                                  (PATH_RAW); one with escapes leaves its raw
//                                  sub-range in path[i] and its decoded length
//                                  in dec_len[i]; a parse error leaves the span
//                                  as the span kernel wrote it (PATH_NONE).  A
//                                  value that is not a string_value needs
//                                  AsString: the span joins the host pass's list.
//   otlp_url_full_unescape_kernel  one lane per span with a dec_len, after the
//                                  scan of dec_len and the arena's regrow: the
//                                  decoded bytes at dec_base + dec_off[i],
//                                  path[i] pointed there, PATH_RAW set.
//
// Every byte is read through ByteReader::at inside the span's payload, which
// the span kernel has walked already (16 bytes of slack after the message).
// The unescape pass writes plain bytes into a region of the arena that no lane
// reads.  No LDS; the atomics are the host list's counter, as in the span
// kernel, and one add per wave to the parsed-span counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_common.hpp"
#include "kernels.hpp"
#include "pb_device.hpp"
#include "url_full.hpp"

namespace ose {
namespace {
using namespace pbdev;

constexpr int kUfThreads = 256;

constexpr uint64_t le8(const char* s) {
  uint64_t v = 0;
  for (int k = 7; k >= 0; k--) v = (v << 8) | (uint8_t)s[k];
  return v;
}
constexpr uint32_t kKeyLen = 8;   // "url.full", "http.url"
constexpr uint64_t kUrlFull = le8("url.full"), kHttpUrl = le8("http.url");

// the parser's byte source: the lane's 16-byte reader over the arena
struct ArenaSrc {
  ByteReader& br;
  __device__ __forceinline__ uint32_t at(uint32_t i) { return br.at(i); }
};

// span i; true: a string value was parsed here
__device__ bool parse_span(const OtlpUrlFullArgs& a, uint64_t i) {
  if (a.host_flag[i]) return false;   // listed by the span kernel: the host pass writes its path
  const uint32_t uf = a.url_flags[i];
  if (!(uf & OSE_URL_HAS_METHOD) || (uf & OSE_URL_PATH_MASK) != OSE_URL_PATH_NONE) return false;
  const uint64_t ref = a.span_ref[i];
  const uint32_t s0 = (uint32_t)ref, s1 = s0 + (uint32_t)(ref >> 32);
  Rd r(a.pb, s0, s1);
  // the value's place of the first url.full and of the first http.url
  bool has_full = false, has_old = false, full_val = false, old_val = false;
  uint32_t full_s = 0, full_l = 0, old_s = 0, old_l = 0;
  uint32_t f, wt;
  while (r.more() && r.tag(f, wt)) {
    uint32_t ps, pl;
    if (f != 9 || wt != 2) { r.skip(wt); continue; }
    if (!r.len(ps, pl)) break;
    // the KeyValue: key (1) and value (2); the span kernel sent a span with
    // either field repeated to the host pass
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
    if (kl != kKeyLen) continue;
    uint64_t key = 0;
    for (uint32_t k = 0; k < 8; k++) key |= (uint64_t)r.br.at(ko + k) << (8 * k);
    if (key == kUrlFull && !has_full) {
      has_full = true; full_val = has_val; full_s = vs; full_l = vl;
      break;   // the first url.full is the source whatever follows
    }
    if (key == kHttpUrl && !has_old) {
      has_old = true; old_val = has_val; old_s = vs; old_l = vl;
    }
  }
  bool host = r.bad;
  if (!host && (has_full || has_old)) {
    const bool hv = has_full ? full_val : old_val;
    const uint32_t vs = has_full ? full_s : old_s, vl = has_full ? full_l : old_l;
    Val v{OSE_ATTR_OTHER, 0, 0, 0};
    if (hv) any_value(r, vs, vs + vl, v);
    if (r.bad || v.type != OSE_ATTR_STR) {
      host = true;   // AsString of an int, double, bool, bytes, array, kvlist or empty value
    } else {
      ArenaSrc src{r.br};
      const urlfull::Result p = urlfull::parse(src, v.off, v.len);
      if (p.outcome == urlfull::kDecoded) {
        a.path[i] = ose_strref{p.off, p.len};   // parked: the unescape pass replaces it
        a.dec_len[i] = p.dec_len;
      } else if (p.outcome != urlfull::kError) {
        a.path[i] = ose_strref{p.off, p.len};
        a.url_flags[i] = (uint8_t)(uf | OSE_URL_PATH_RAW);
      }
      return true;
    }
  }
  if (host) {
    a.host_flag[i] = 1;
    const uint32_t slot = atomicAdd(a.host_count, 1u);
    if (slot < a.host_cap) a.host_list[slot] = (uint32_t)i;
  }
  return false;
}

__global__ __launch_bounds__(kUfThreads) void otlp_url_full_kernel(OtlpUrlFullArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kUfThreads;
  // the trip count is the workgroup's: every lane of a wave reaches the ballot
  for (uint64_t i0 = (uint64_t)blockIdx.x * kUfThreads; i0 < a.n_spans; i0 += stride) {
    const uint64_t i = i0 + threadIdx.x;
    bool parsed = false;
    if (i < a.n_spans) {
      a.dec_len[i] = 0;
      parsed = parse_span(a, i);
    }
    const uint64_t m = __ballot(parsed);
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(a.parsed, (uint32_t)__popcll(m));
  }
}

__global__ __launch_bounds__(kUfThreads) void otlp_url_full_unescape_kernel(OtlpUrlFullArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kUfThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kUfThreads + threadIdx.x; i < a.n_spans; i += stride) {
    const uint32_t n = a.dec_len[i];
    if (!n) continue;
    const ose_strref raw = a.path[i];
    const uint32_t at = a.dec_base + a.dec_off[i];
    ByteReader br(a.pb);
    ArenaSrc src{br};
    urlfull::unescape_into(src, raw.off, raw.len, a.out + at);
    a.path[i] = ose_strref{at, n};
    a.url_flags[i] = (uint8_t)(a.url_flags[i] | OSE_URL_PATH_RAW);
  }
}

}  // namespace

void launch_otlp_url_full(const OtlpUrlFullArgs& a, hipStream_t st) {
  const uint64_t blocks = std::min<uint64_t>((a.n_spans + kUfThreads - 1) / kUfThreads, 16384);
  if (blocks) hipLaunchKernelGGL(otlp_url_full_kernel, dim3((uint32_t)blocks), dim3(kUfThreads), 0, st, a);
}

void launch_otlp_url_full_unescape(const OtlpUrlFullArgs& a, hipStream_t st) {
  const uint64_t blocks = std::min<uint64_t>((a.n_spans + kUfThreads - 1) / kUfThreads, 16384);
  if (blocks) hipLaunchKernelGGL(otlp_url_full_unescape_kernel, dim3((uint32_t)blocks), dim3(kUfThreads), 0, st, a);
}

}  // namespace ose
