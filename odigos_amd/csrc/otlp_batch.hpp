// otlp_batch.hpp — the decoded OTLP batch (ose_otlp_batch), as its three host
// files share it: otlp_host.cpp makes and owns it (decode, the accessors,
// release), otlp_condattr_host.cpp adds odigosconditionalattributes' columns
// during the decode, otlp_encode_host.cpp re-encodes from it.  Internal to
// those three.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "engine_internal.hpp"
#include "kernels.hpp"
#include "otlp_encode.hpp"
#include "slab.hpp"

namespace ose {

struct DevBuf {   // grow-only device (or pinned host) buffer
  uint8_t* p = nullptr;
  size_t cap = 0;
  bool host = false;
  int need(size_t bytes);   // at least `bytes`; contents are lost when it grows (otlp_host.cpp has the growth rule)
  ~DevBuf() {
    if (p) { if (host) (void)hipHostFree(p); else (void)hipFree(p); }
  }
};

struct OtlpBatchImpl {
  Engine* e = nullptr;
  ose_columns cols{};
  DevBuf arena, slab, stage, fixdev;   // device arena; device columns; pinned staging; host-pass records
  std::vector<std::vector<std::pair<std::string, std::string>>> attrsets;
  uint32_t host_spans = 0;
  // engine option otlp_url_full (ose_otlp_url_full_counts): the spans whose
  // url.full / http.url the GPU parsed, the decoded path bytes it wrote
  uint64_t url_full_counts[2] = {0, 0};
  // which path the decode took (ose_otlp_walk_info): [0] the GPU chain linked,
  // [1] resource-table misses, [2] of them entered into the table's key space
  // (one Resource field or none), [3] scopes the host sized, [4] the scope
  // redo, [5] the resource redo, [6] the span kernel (1 LDS-staged, 2 HBM),
  // [7] the arena regrown
  uint32_t walk_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double t_ms[5] = {0, 0, 0, 0, 0};   // copy-in, walk, columns upload, span kernel (+ sync), host pass
  // for ose_otlp_encode: the caller's message and where its parts are
  const uint8_t* pb = nullptr;
  size_t pb_len = 0;
  std::vector<uint64_t> span_ref;
  OtlpLayout lay;
  // with the scopes walked on the GPU, span_ref and the scopes' span0 / hdr
  // / schema are on the device until ose_otlp_encode (or the host pass)
  // brings them back
  bool layout_on_host = true;
  DevBuf sslab;   // scope-level device arrays
  DevBuf rslab, setbuf, cslab;   // resource-level device arrays; attribute-set compaction; the GPU chain walk
  uint64_t* d_res_ref = nullptr;   // the ResourceSpans refs (lay.res_ref is filled from it on demand)
  bool res_on_device = false;   // res_scope0 / scope_ref / attr_res live on the device (rslab, sslab)
  uint32_t* d_res_scope0 = nullptr;
  uint64_t* d_scope_ref = nullptr;
  uint64_t* d_attr_res = nullptr;
  uint64_t* d_span_ref = nullptr;
  uint32_t *d_span_res = nullptr, *d_span0 = nullptr;
  uint64_t *d_hdr = nullptr, *d_schema = nullptr;
  OtlpScopeArgs sargs{};   // the GPU scope walk's arrays (pass 2 reuses them)
  // the GPU encoder (encode_kernel.hip): the span refs in HBM (always), the
  // scope level there when the GPU walked it; its workspace and outputs
  uint64_t* d_spans = nullptr;
  bool scopes_dev = false;
  DevBuf eslab, eout, emisc;
  DevBuf seth;   // pinned: the resource pass's attribute-set scan words and ids (read after the scope pass's wait)
  // a batch released by a groupbytrace store (ose_gbt_release_otlp): the
  // store owns it, `arena` is the released message buffer and every layout
  // array is the store's; relhost takes the buffer when the host encoder runs
  bool released = false;
  DevBuf relhost;
  // engine option otlp_condattr (on at the decode: ca_on): the stage's columns
  // (ose_otlp_condattr_columns) for the engine's ca_keys keys, in a slab of
  // their own; cafix takes the host pass's entries
  bool ca_on = false;
  uint32_t ca_keys = 0;
  ose_condattr_columns ca{};
  DevBuf caslab, cafix;
  OtlpBatchImpl() { stage.host = true; emisc.host = true; seth.host = true; relhost.host = true; }
};

// The host-pass list the span kernels (span, sqlop, condattr) add to, and its
// four fields on any of their argument blocks.
struct HostList { uint8_t* flag = nullptr; uint32_t *count = nullptr, *list = nullptr; uint32_t cap = 0; };
template <class Args>
void set_host_list(Args& a, const HostList& h) {
  a.host_flag = h.flag;
  a.host_count = h.count;
  a.host_list = h.list;
  a.host_cap = h.cap;
}

// What the other two need of the decoder's file (otlp_host.cpp).
// span refs and the scopes' span0 / header / schema refs back to the host
int layout_to_host(OtlpBatchImpl* b, hipStream_t st);
// an arena of at least `want` bytes: when it grows, the first `keep` bytes move with it
int regrow_arena(OtlpBatchImpl* b, size_t keep, size_t want, hipStream_t st);
// Engine option otlp_condattr (otlp_condattr_host.cpp), called by decode():
// the stage's span columns behind the span kernels, and the rest after the
// host pass (`list`: its spans, `host_list` the same on the device).
int condattr_spans(Engine* e, OtlpBatchImpl* b, uint64_t n, const uint64_t* span_ref, const HostList& hl,
                   hipStream_t st);
int condattr_finish(Engine* e, OtlpBatchImpl* b, const uint8_t* pb, const std::vector<uint32_t>& list,
                    const uint32_t* host_list, hipStream_t st);
// The host walk of `pb` with a default columniser context (the CPU test
// seams): the span refs, the layout, and pdata's size of every span as the
// decoder would compute it.  OSE_EINVAL on a malformed message.
int otlp_host_walk_sizes(const uint8_t* pb, size_t len, std::vector<uint64_t>& span_ref, OtlpLayout& lay,
                         std::vector<uint32_t>& span_size);

}  // namespace ose
