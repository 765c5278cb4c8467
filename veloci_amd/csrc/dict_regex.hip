// k_dict_regex — regex leaves: one lane per dictionary term walks the probe's DFA (regex_dfa.hpp) over the term's code points,
//     state = next[state + class(code point)]        (states are stored premultiplied by the number of classes)
// and the term matches when the walk ENDS in an accepting state (with starts_with the host made the accepting state absorbing).  Case is in
// the DFA's atoms already, so the walk always reads the RAW image (u16 or u32 per Dictionary::char_bytes).
//
//   grid.x   a block serves kRegexRounds rounds of 256 consecutive terms     grid.y   the probe
//   LDS      the probe's tables, loaded once per block: next[], the class of every code point below 128 (direct), the class of every non-ASCII
//            code point of the dictionary's alphabet beside the sorted alphabet itself (binary search: an LDS read per step, no HBM image per
//            character); the round's contiguous stretch of the image, staged with 16-byte loads per lane (a term that reaches beyond the
//            stage is walked from HBM, as in k_dict_scan)
//   output   DictMatch{probe, term, 0} through k_dict_scan's counter-and-capacity protocol: ballot, prefix count, one atomic per wave
//
// Two table sizes, each a kernel with static LDS: vqregex::kLdsTableBytes (two blocks per CU) and kLdsTableBytesSmall (eight).
#include "kernel_common.hpp"
#include "kernels.hpp"
#include "regex_dfa.hpp"

namespace vq {

constexpr uint32_t kRegexStageBytes = 8192;  // a round's 256 terms staged in LDS: 2 x 16 bytes per lane
constexpr uint32_t kRegexRounds = 8;
constexpr uint32_t kRegexAreaSlack = 32;     // the two sub-tables start on 16-byte boundaries
static_assert(vqregex::kLdsTableBytes + kRegexAreaSlack + kRegexStageBytes + 257 * 4 + 64 <= 80 * 1024, "two blocks of k_dict_regex per CU");
static_assert(vqregex::lds_table_bytes(vqregex::kMaxStates, 1, 0) <= vqregex::kLdsTableBytes, "the state cap is the tighter one for a one-class DFA");
static_assert(vqregex::kLdsTableBytes / 2 < 65536, "premultiplied states fit 16 bits");

template <class CharT, bool STAGED>
__device__ __forceinline__ uint32_t regex_walk(uint32_t state, const CharT* text, uint32_t n, const uint16_t* next, const uint16_t* ascii, const uint16_t* acls,
                                               const uint32_t* acp, uint32_t n_alpha) {
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t cp;
        if constexpr (STAGED) cp = text[i];
        else cp = as_global(text)[i];
        uint32_t c;
        if (cp < 128u) c = ascii[cp];
        else {
            uint32_t lo = 0, hi = n_alpha;  // first alphabet entry >= cp (it is in there: the alphabet was collected from this image)
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (acp[mid] < cp) lo = mid + 1u;
                else hi = mid;
            }
            c = lo < n_alpha ? acls[lo] : 0u;
        }
        state = next[state + c];
    }
    return state;
}

template <class CharT, uint32_t TABLE_BYTES>
__global__ __launch_bounds__(256) void k_dict_regex(const RegexProbeD* __restrict__ probes, const uint16_t* __restrict__ pool, const uint32_t* __restrict__ alpha,
                                                    uint32_t n_alpha, uint32_t probe_base, const uint32_t* __restrict__ off, const CharT* __restrict__ chars,
                                                    uint32_t num_terms, uint32_t* __restrict__ out_count, uint32_t out_cap, DictMatch* __restrict__ out) {
    constexpr uint32_t kStage = kRegexStageBytes / sizeof(CharT);
    __shared__ u32x4 area[(TABLE_BYTES + kRegexAreaSlack) / 16];
    __shared__ u32x4 stage4[kRegexStageBytes / 16];
    __shared__ uint32_t soff[257];  // a round's term offsets, relative to its first code point
    const uint32_t tid = threadIdx.x;
    const VQ_CONST RegexProbeD* P = as_const<RegexProbeD>(probes + blockIdx.y);
    const uint32_t tab_off = P->tab_off, n_next = P->n_next, start = P->start, first_accept = P->first_accept;
    const uint32_t words16 = regex_words16(n_next, n_alpha);
    if (words16 * 2u + n_alpha * 4u > TABLE_BYTES + kRegexAreaSlack || start >= n_next) return;  // (uniform; the host never sends such a probe)
    {  // the probe's tables: [next | class below 128 | class of alphabet[k]] as u16 (16-byte groups: tab_off and words16 are multiples of 8) ...
        const VQ_GLOBAL u32x4* src = (const VQ_GLOBAL u32x4*)(pool + tab_off);
        for (uint32_t k = tid; k < words16 / 8u; k += 256u) area[k] = src[k];
        // ... and the non-ASCII part of the dictionary's alphabet behind them
        uint32_t* acp_w = reinterpret_cast<uint32_t*>(area) + words16 / 2u;
        for (uint32_t k = tid; k < n_alpha; k += 256u) acp_w[k] = as_global(alpha)[k];
    }
    const uint16_t* next = reinterpret_cast<const uint16_t*>(area);
    const uint16_t* ascii = next + n_next;
    const uint16_t* acls = ascii + 128;
    const uint32_t* acp = reinterpret_cast<const uint32_t*>(area) + words16 / 2u;
    const CharT* stage = reinterpret_cast<const CharT*>(stage4);
    const unsigned long long total_bytes = (unsigned long long)off[num_terms] * sizeof(CharT);
    const uint32_t first_t0 = blockIdx.x * kRegexRounds * 256u;
    for (uint32_t round = 0; round < kRegexRounds; ++round) {
        const uint32_t t0 = first_t0 + round * 256u;
        if (t0 >= num_terms) break;  // uniform
        const uint32_t t_end = t0 + 256u < num_terms ? t0 + 256u : num_terms;
        const uint32_t base = off[t0];  // (uniform)
        __syncthreads();                // the previous round's readers of `stage` / `soff` are done (round 0: nothing)
        soff[tid] = off[t0 + tid <= num_terms ? t0 + tid : num_terms] - base;  // off[] has num_terms + 1 entries
        if (tid == 0) soff[256] = off[t0 + 256u <= num_terms ? t0 + 256u : num_terms] - base;
        // the stretch from the 16-byte boundary at or below its first code point: `shift` elements of the previous round's come first
        const unsigned long long byte_lo = (unsigned long long)base * sizeof(CharT), abase = byte_lo & ~15ull;
        const uint32_t shift = (uint32_t)(byte_lo - abase) / (uint32_t)sizeof(CharT);
#pragma unroll
        for (uint32_t k = 0; k < kRegexStageBytes / 16u / 256u; ++k) {
            const unsigned long long a = abase + (unsigned long long)(k * 256u + tid) * 16u;
            // (the image is allocated with 16 bytes of slack: a vector that starts inside it ends inside the allocation)
            if (a < total_bytes) stage4[k * 256u + tid] = *(const VQ_GLOBAL u32x4*)((const VQ_GLOBAL uint8_t*)chars + a);
        }
        __syncthreads();
        bool match = false;
        if (t0 + tid < t_end) {
            const uint32_t b = soff[tid], n = soff[tid + 1] - b;
            uint32_t state;
            if (shift + b + n <= kStage) state = regex_walk<CharT, true>(start, stage + shift + b, n, next, ascii, acls, acp, n_alpha);
            else state = regex_walk<CharT, false>(start, chars + base + b, n, next, ascii, acls, acp, n_alpha);
            match = state >= first_accept;
        }
        const unsigned long long m = __ballot(match);
        if (m) {  // uniform per wave: one reservation for the wave's matches
            uint32_t wbase = 0u;
            if (lane_id() == 0u) wbase = atomicAdd(out_count, (uint32_t)__popcll(m));
            wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
            if (match) {
                const uint32_t pos = wbase + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
                if (pos < out_cap) out[pos] = DictMatch{probe_base + blockIdx.y, t0 + tid, 0u};
            }
        }
    }
}

template <class CharT, uint32_t TABLE_BYTES>
static void launch_regex_form(hipStream_t st, const RegexProbeD* d_probes, const uint16_t* pool, const uint32_t* alpha, uint32_t n_alpha, uint32_t probe_base,
                              uint32_t n_probes, const uint32_t* off, const void* chars, uint32_t num_terms, uint32_t* out_count, uint32_t out_cap, DictMatch* out) {
    const uint32_t blocks = (num_terms + 256u * kRegexRounds - 1u) / (256u * kRegexRounds);
    for (uint32_t p0 = 0; p0 < n_probes; p0 += 65535u) {  // grid.y
        const uint32_t np = n_probes - p0 < 65535u ? n_probes - p0 : 65535u;
        hipLaunchKernelGGL((k_dict_regex<CharT, TABLE_BYTES>), dim3(blocks, np), dim3(256), 0, st, d_probes + p0, pool, alpha, n_alpha, probe_base + p0, off,
                           static_cast<const CharT*>(chars), num_terms, out_count, out_cap, out);
    }
}

void launch_dict_regex(hipStream_t st, uint32_t char_bytes, bool small_tables, const RegexProbeD* d_probes, const uint16_t* pool, const uint32_t* alpha, uint32_t n_alpha,
                       uint32_t probe_base, uint32_t n_probes, const uint32_t* off, const void* chars, uint32_t num_terms, uint32_t* out_count, uint32_t out_cap,
                       DictMatch* out) {
    if (!n_probes || !num_terms) return;
    if (char_bytes == 4) {
        if (small_tables)
            launch_regex_form<uint32_t, vqregex::kLdsTableBytesSmall>(st, d_probes, pool, alpha, n_alpha, probe_base, n_probes, off, chars, num_terms, out_count, out_cap, out);
        else launch_regex_form<uint32_t, vqregex::kLdsTableBytes>(st, d_probes, pool, alpha, n_alpha, probe_base, n_probes, off, chars, num_terms, out_count, out_cap, out);
    } else {
        if (small_tables)
            launch_regex_form<uint16_t, vqregex::kLdsTableBytesSmall>(st, d_probes, pool, alpha, n_alpha, probe_base, n_probes, off, chars, num_terms, out_count, out_cap, out);
        else launch_regex_form<uint16_t, vqregex::kLdsTableBytes>(st, d_probes, pool, alpha, n_alpha, probe_base, n_probes, off, chars, num_terms, out_count, out_cap, out);
    }
}

}  // namespace vq
