// TEST INFRASTRUCTURE — the regex scan's launcher for the stubbed device layer (see hip_stub.cpp): it throws like every other stubbed launcher
// (with VQ_STUB_NOOP_LAUNCH=1 it does nothing).  With VQ_STUB_DICT_SCAN=1 it answers the probes on the host instead, walking the very tables
// k_dict_regex would read ("device" memory is host memory here) and writing DictMatch records through the same counter-and-capacity protocol:
// what the host side made of a pattern — DFA, premultiplied states, class tables, alphabet — is then checked end to end without a GPU.
// Linked next to hip_stub.cpp into the CPU sanitizer and host-stub builds only.
#include <cstdlib>
#include <string>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
void launch_dict_regex(hipStream_t, uint32_t char_bytes, bool small_tables, const RegexProbeD* probes, const uint16_t* pool, const uint32_t* alpha, uint32_t n_alpha,
                       uint32_t probe_base, uint32_t n_probes, const uint32_t* off, const void* chars, uint32_t num_terms, uint32_t* out_count, uint32_t out_cap,
                       DictMatch* out) {
    if (!std::getenv("VQ_STUB_DICT_SCAN")) {
        if (std::getenv("VQ_STUB_NOOP_LAUNCH")) return;
        throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: k_dict_regex"));
    }
    for (uint32_t p = 0; p < n_probes; ++p) {
        const RegexProbeD& P = probes[p];
        const uint64_t lds = uint64_t(regex_words16(P.n_next, n_alpha)) * 2 + uint64_t(n_alpha) * 4;
        if (lds > (small_tables ? vqregex::kLdsTableBytesSmall : vqregex::kLdsTableBytes) + 32u || P.start >= P.n_next)
            throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_dict_regex (stub): a probe whose tables the kernel would refuse");
        const uint16_t* next = pool + P.tab_off;
        const uint16_t* ascii = next + P.n_next;
        const uint16_t* acls = ascii + 128;
        for (uint32_t t = 0; t < num_terms; ++t) {
            uint32_t state = P.start;
            for (uint32_t i = off[t]; i < off[t + 1]; ++i) {
                const uint32_t cp = char_bytes == 4 ? static_cast<const uint32_t*>(chars)[i] : static_cast<const uint16_t*>(chars)[i];
                uint32_t c;
                if (cp < 128u) c = ascii[cp];
                else {
                    uint32_t lo = 0, hi = n_alpha;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (alpha[mid] < cp) lo = mid + 1u;
                        else hi = mid;
                    }
                    c = lo < n_alpha ? acls[lo] : 0u;
                }
                if (state + c >= P.n_next) throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_dict_regex (stub): a transition outside the table");
                state = next[state + c];
            }
            if (state >= P.first_accept) {
                const uint32_t pos = (*out_count)++;
                if (pos < out_cap) out[pos] = DictMatch{probe_base + p, t, 0u};
            }
        }
    }
}
}  // namespace vq
