// sqlop_san.cpp — stand-alone driver of the SQL operation classifier
// (odigos_amd/csrc/sqlop_device.hpp, the source sqlop_kernel's general path and
// osehost_sqlop_detect compile) for an ASan + UBSan build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// tests/fuzz/run_sqlop_san.py writes the cases (the golden ones and seeded
// random strings with the codes of the Python restatement), builds and runs it.
// Each query is copied into a heap block of exactly its length, so a read one
// byte past the string is an ASan error.  Input: one case per line,
// "<hex bytes or -> <expected OSE_SQLOP_* code>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../odigos_amd/csrc/sqlop_device.hpp"

static int hexval(char c) { return c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10; }

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: sqlop_san CASES\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::string hex;
  unsigned want = 0;
  uint64_t n_cases = 0, bad = 0;
  while (in >> hex >> want) {
    if (hex == "-") hex.clear();
    const size_t len = hex.size() / 2;
    uint8_t* q = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    for (size_t k = 0; k < len; k++) q[k] = (uint8_t)(hexval(hex[2 * k]) * 16 + hexval(hex[2 * k + 1]));
    // the bytes exactly as long as the string: the 1-byte block of an empty one is never read
    uint8_t* exact = len ? static_cast<uint8_t*>(std::malloc(len)) : nullptr;
    for (size_t k = 0; k < len; k++) exact[k] = q[k];
    ose::sqlop::HostBytes rd{exact};
    const uint32_t got = ose::sqlop::detect(rd, (uint32_t)len);
    if (got != want) {
      if (bad++ < 10) std::fprintf(stderr, "case %llu (%s): got %u, want %u\n", (unsigned long long)n_cases, hex.c_str(), got, want);
    }
    std::free(exact);
    std::free(q);
    n_cases++;
  }
  std::printf("sqlop_san: %llu cases, %llu mismatches\n", (unsigned long long)n_cases, (unsigned long long)bad);
  return bad ? 1 : (n_cases ? 0 : 2);
}
