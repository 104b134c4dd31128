// condattr_san.cpp — stand-alone driver of the odigosconditionalattributes
// steps (odigos_amd/csrc/condattr_device.hpp, the source condattr_kernel.hip
// and osehost_condattr_span compile) for an ASan + UBSan build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// tests/fuzz/run_condattr_san.py writes the case file (the compiled blob, the
// columns and the results of the Python restatement), builds and runs it.
// Every column is copied into a heap block of exactly its length (the arena
// exactly arena_bytes long), so a read one byte past a column or a string is
// an ASan error.  Case file: blocks of [u64 length][bytes] in the order read
// below.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "../../odigos_amd/csrc/condattr_device.hpp"

static std::ifstream in;

static void* block(uint64_t* len = nullptr) {
  uint64_t n = 0;
  in.read(reinterpret_cast<char*>(&n), 8);
  if (!in) { std::fprintf(stderr, "short case file\n"); std::exit(2); }
  void* p = std::malloc(n ? n : 1);
  if (n) in.read(static_cast<char*>(p), (std::streamsize)n);
  if (n == 0) { std::free(p); p = nullptr; }
  if (len) *len = n;
  return p;
}

int main(int argc, char** argv) {
  using namespace ose::condattr;
  if (argc < 2) { std::fprintf(stderr, "usage: condattr_san CASES\n"); return 2; }
  in.open(argv[1], std::ios::binary);
  if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint64_t n_batches = 0, spans = 0, bad = 0;
  for (;;) {
    uint64_t dims[4];
    in.read(reinterpret_cast<char*>(dims), sizeof dims);   // n_spans, n_resources, n_scopes, arena_bytes
    if (!in) break;
    std::vector<void*> owned;
    auto take = [&](uint64_t* len = nullptr) { void* p = block(len); owned.push_back(p); return p; };
    const uint8_t* blob = static_cast<const uint8_t*>(take());
    ose_condattr_columns c{};
    c.n_spans = dims[0]; c.n_resources = (uint32_t)dims[1]; c.n_scopes = (uint32_t)dims[2]; c.arena_bytes = dims[3];
    c.arena = static_cast<const uint8_t*>(take());
    c.scope = static_cast<const uint32_t*>(take());
    c.scope_resource = static_cast<const uint32_t*>(take());
    c.scope_name = static_cast<const ose_strref*>(take());
    c.span_has = static_cast<const uint8_t*>(take());
    c.span_val = static_cast<const ose_strref*>(take());
    c.span_kv_size = static_cast<const uint32_t*>(take());
    c.scope_has = static_cast<const uint8_t*>(take());
    c.scope_val = static_cast<const ose_strref*>(take());
    c.res_has = static_cast<const uint8_t*>(take());
    c.res_val = static_cast<const ose_strref*>(take());
    c.span_size = static_cast<const uint32_t*>(take());
    // expected: per target and span 0 = KEEP else 1, the value bytes' FNV-1a
    // and length; then span_size_out
    const uint8_t* want_put = static_cast<const uint8_t*>(take());
    const uint32_t* want_hash = static_cast<const uint32_t*>(take());
    const uint32_t* want_len = static_cast<const uint32_t*>(take());
    const uint32_t* want_size = static_cast<const uint32_t*>(take());
    const View v = view(blob);
    const uint64_t n = c.n_spans, U = v.h->n_targets;
    std::vector<uint8_t> src(U * n + 1, 0xEE);
    std::vector<ose_strref> val(U * n + 1);
    std::vector<uint32_t> size_out(n + 1), scratch(scratch_words(*v.h, c.n_scopes) + 1);
    ose_condattr_outputs o{};
    o.src = src.data(); o.val = val.data(); o.span_size_out = size_out.data();
    for (uint32_t s = 0; s < c.n_scopes; s++) scope_step<HostEnv>(v, c, scratch.data(), s);
    for (uint64_t i = 0; i < n; i++) span_step<HostEnv>(v, c, o, scratch.data(), i);
    for (uint64_t i = 0; i < n; i++) {
      bool ok = size_out[i] == want_size[i];
      for (uint64_t u = 0; u < U && ok; u++) {
        const uint64_t x = u * n + i;
        if ((src[x] != OSE_CA_KEEP) != (want_put[x] != 0)) ok = false;
        else if (src[x] != OSE_CA_KEEP) {
          const uint8_t* base = src[x] == OSE_CA_CONFIG ? v.strings : c.arena;
          ok = val[x].len == want_len[x] && hash_bytes_host(base + val[x].off, val[x].len) == want_hash[x];
        }
      }
      if (!ok && bad++ < 10) std::fprintf(stderr, "batch %llu span %llu differs\n", (unsigned long long)n_batches, (unsigned long long)i);
    }
    spans += n;
    n_batches++;
    for (void* p : owned) std::free(p);
  }
  std::printf("condattr_san: %llu batches, %llu spans, %llu mismatches\n", (unsigned long long)n_batches,
              (unsigned long long)spans, (unsigned long long)bad);
  return bad ? 1 : (n_batches ? 0 : 2);
}
