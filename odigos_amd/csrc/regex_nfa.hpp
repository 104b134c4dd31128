// regex_nfa.hpp — a Go regexp as an NFA program: the tables of the bit-set
// simulation regex_nfa_device.hpp runs, for the regexps whose DFA passes
// Dfa::kMaxStates / kMaxTableBytes or needs more than 255 rune classes
// (odigosurltemplate custom_ids and rule regexps; regexp.Compile takes them,
// config.go:146-155, and Go matches them with a Pike VM).
//
// Built from the same parse, Thompson NFA, rune classes and EmptyOpContext
// types as the DFA (regex_dfa.cpp prepare()), so both routes decide every
// input alike; invalid UTF-8 is U+FFFD of width 1 here too.  Per distinct
// context (context(prev, next) masked by the empty-width ops the program
// uses: one table for a pattern without assertions, at most 16) every entry
// (the M rune instructions and the start) has its epsilon closure as a sparse
// successor row (CSR) and a match bit; per rune class a bit set of the rune
// instructions whose set holds it.  Class ids are 16 bits wide.
//
// The bound: one program's tables stay within kMaxTableBytes (the DFA's
// table cap), and the parser compiles at most 100,000 instructions
// ("expression too large").  ^(?:a|b)*a(?:a|b){1000}$, Go's largest repeat
// count, is about 2,000 rune instructions and 100 KB.  Matching is linear in
// pattern x input; what passes the bound is TooLarge.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "devcfg.hpp"
#include "regex_dfa.hpp"

namespace ose {

struct NfaProgram {
  static constexpr uint64_t kMaxTableBytes = Dfa::kMaxTableBytes;
  uint32_t m = 0;                          // rune instructions
  uint32_t nclasses = 0, nctx = 0;
  uint8_t ctx_of[16] = {};                 // [previous type * 4 + next type]
  uint16_t ascii[128] = {};
  std::vector<uint32_t> hi_lo, hi_hi, hi_cls;
  std::vector<uint8_t> cls_type;           // [nclasses]
  std::vector<uint32_t> row;               // [nctx][m + 2]
  std::vector<uint32_t> succ;
  std::vector<uint32_t> match;             // [nctx][(m + 32) / 32]
  std::vector<uint32_t> in_class;          // [nclasses][(m + 31) / 32, >= 1]
  uint32_t words() const { return m ? (m + 31) / 32 : 1; }
};

// Syntax / Unsupported as compile_dfa; TooLarge past the NFA bound (err names
// it).  max_table_bytes lowers the cap (never above kMaxTableBytes).
// (Defined in regex_dfa.cpp, beside the NFA it reads.)
RegexStatus compile_nfa(const std::string& pattern, NfaProgram& out, std::string& err,
                        uint64_t max_table_bytes = NfaProgram::kMaxTableBytes);

// The relocatable device image of a program (NfaDev and its sections; what
// the URL blob holds, 16-byte aligned).
std::vector<uint8_t> nfa_image(const NfaProgram& p);

// Host-side evaluation of an image through regex_nfa_device.hpp's match().
bool nfa_match(const std::vector<uint8_t>& image, const uint8_t* s, size_t n);

}  // namespace ose
