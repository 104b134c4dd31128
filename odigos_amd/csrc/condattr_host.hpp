// condattr_host.hpp — odigosconditionalattributes: the config compiled into
// the blob of condattr_device.hpp, with the key and target numbering of the
// ABI (include/odigos_amd.h).  ose_engine_create and the host processors
// compile with the same function, so both number alike.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "config.hpp"

namespace ose {

struct CondAttrCompiled {
  std::vector<uint8_t> blob;              // condattr::Header ... strings, 32 bytes of slack
  std::vector<std::string> keys;          // key k's bytes
  std::vector<uint32_t> key_target;       // its target, or OSE_NONE
  std::vector<uint32_t> target_key;       // target u's key
  uint32_t n_rules = 0;
  uint32_t strings_off = 0, string_bytes = 0;
};

// 0, or OSE_ENOTSUP (message in ose_last_error) for a config past a bound:
// the tables index with 32 bits, so the blob must stay below 4 GiB.
int compile_condattr(const CondAttrConfig& cfg, CondAttrCompiled& out);

}  // namespace ose
