// Regex leaves on the device: a pattern compiled to a DFA over the code points of ONE dictionary (k_dict_regex walks it, one lane per term).
//
// The compiler implements only the STRUCTURE of a pattern — concatenation, `|`, groups, `* + ? {m} {m,} {m,n}` and their lazy forms.  Which
// characters an atom (a literal, `.`, a bracket expression, `\d \D \w \W \s \S`) matches is asked of std::wregex itself, atom by atom and code
// point by code point of the dictionary's alphabet, with the flags of the leaf: icase, `.`, ranges and the C locale's classes are libstdc++'s
// own answers, not restated here.  Everything outside that structure is declined with a reason and stays on the host route
// (regex_candidates, term_lookup.cpp), which is also the yardstick: same match set, same errors.
//
// Stand-alone on purpose (no HIP, no engine headers): tests/native/regex_dfa_check.cpp links it alone, under the sanitizers.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace vqregex {

constexpr uint32_t kMaxStates = 4096;         // DFA states of a probe; more: host route
constexpr uint32_t kMaxAlphabet = 65535;      // distinct code points of a dictionary; more: host route
constexpr uint32_t kMaxNfaStates = 1u << 15;  // Thompson states after the expansion of `{m,n}`; more: host route
// LDS of k_dict_regex given to ONE probe's tables: u16 next[states][classes], the class of every code point below 128 (256 B) and, per
// non-ASCII code point of the alphabet, the code point (4 B) and its class (2 B).  With the staging buffer two workgroups stay resident per CU.
constexpr uint32_t kLdsTableBytes = 68u * 1024u;
constexpr uint32_t kLdsTableBytesSmall = 8u * 1024u;  // probes under this size run in the small-table form of the kernel (8 workgroups per CU)

// LDS bytes the tables of a probe take (see kLdsTableBytes)
constexpr uint64_t lds_table_bytes(uint64_t states, uint64_t classes, uint64_t non_ascii) { return 2u * states * classes + 256u + 6u * non_ascii; }

struct AtomCache {  // of one dictionary: (atom text, icase) -> which code points of the alphabet the atom matches
    std::mutex mu;
    std::map<std::pair<std::wstring, bool>, std::shared_ptr<const std::vector<uint8_t>>> members;
};

struct Dfa {
    uint32_t n_states = 0, n_classes = 0;
    uint32_t start = 0;
    uint32_t first_accept = 0;   // states [first_accept, n_states) accept
    std::vector<uint16_t> next;  // [n_states][n_classes]
    std::vector<uint16_t> cls;   // class of alphabet[i]
};
struct Compiled {
    bool device = false;  // false: host route, `reason` says why
    std::string reason;
    Dfa dfa;
};

// `alphabet`: the dictionary's distinct code points, ascending.  The caller has constructed the leaf's std::wregex objects before (an invalid
// pattern never gets here).  starts_with: accepting states absorb (regex_search); else the walk has to END in one (regex_match of the
// `[\s\S]*?(?:pattern)` wrapper: some suffix matches).
Compiled compile(const std::vector<uint32_t>& pattern, bool icase, bool starts_with, const std::vector<uint32_t>& alphabet, AtomCache& cache);

// the walk k_dict_regex does, on the host (code points outside the alphabet never occur in the dictionary's own terms: they reject)
bool accepts(const Dfa& dfa, const std::vector<uint32_t>& alphabet, const uint32_t* cps, size_t n);

}  // namespace vqregex
