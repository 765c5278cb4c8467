// TEST INFRASTRUCTURE — the launchers of veloci_amd/csrc/docset_aggs.hip for the host builds that stub the device layer (see hip_stub.cpp).
// Without VQ_STUB_DICT_SCAN they throw like every other launcher.  With VQ_STUB_DICT_SCAN=1 they are answered on the host by plain loops over the
// kernels' own operands — the descriptors, the columns and presence words, the set's padded ids or its membership bitmap, the value_id_to_anchor
// table, the edge keys — into the kernels' own state layout (kernels.hpp), so that the host side of the aggregations (parsing, column resolution,
// the edges' move to keys, the state area, the sum over the shards with the min / max agreement, the rounding of the exact sum, the error paths)
// runs end to end without a GPU.  What a kernel relies on and the host must guarantee is checked here and thrown when it does not hold.  Never
// linked into the product library.
#include <cstdlib>
#include <string>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
static void agg_needs_host_loop(const char* what) {
    if (!std::getenv("VQ_STUB_DICT_SCAN")) throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: ") + what);
}
static void agg_bad(const char* kernel, const char* what) { throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string(kernel) + " (stub): " + what); }
static bool agg_bit_of(const uint32_t* words, uint64_t at) { return (words[at >> 5] >> (at & 31u)) & 1u; }
static void agg_check(const char* kernel, const DocsetAggD& a, const unsigned long long* state, const uint32_t* mm) {
    if (!a.values) agg_bad(kernel, "an aggregation without a column");
    if (a.n_edges > kAggMaxEdges) agg_bad(kernel, "more edges than the LDS table holds");
    for (uint32_t i = 0; i < a.n_edges; ++i) {
        if (a.edges[i] < kRangeKeyMin || a.edges[i] > kRangeKeyMax) agg_bad(kernel, "an edge key among the NaNs");
        if (i && a.edges[i - 1] > a.edges[i]) agg_bad(kernel, "edge keys that descend");
    }
    if (a.mm_off & 1u) agg_bad(kernel, "a min / max pair at an odd offset");
    (void)state;
    (void)mm;
}
// one present value into the state: the restatement of agg_value and of the limb arithmetic
static void agg_add(const DocsetAggD& a, uint32_t bits, unsigned long long* state, uint32_t* mm) {
    unsigned long long* s = state + a.state_off;
    const uint32_t mag = bits & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) {
        ++s[kAggNan];
        return;
    }
    ++s[kAggCount];
    const uint32_t key = range_key(bits);
    if (key < mm[a.mm_off]) mm[a.mm_off] = key;
    if (key > mm[a.mm_off + 1]) mm[a.mm_off + 1] = key;
    if (a.n_edges) {
        uint32_t b = 0;
        while (b < a.n_edges && a.edges[b] <= key) ++b;
        ++s[kAggBuckets + b];
    }
    if (mag == 0x7F800000u) {
        ++s[(bits >> 31) ? kAggNegInf : kAggPosInf];
        return;
    }
    if (!mag) return;
    const uint32_t be = mag >> 23, m = be ? ((mag & 0x007FFFFFu) | 0x00800000u) : mag, sh = (be ? be : 1u) - 1u;
    const unsigned long long w = (unsigned long long)m << (sh & 31u);
    unsigned long long* limb = s + kAggLimbs + (bits >> 31) * kAggLimbsPerSign;
    limb[sh >> 5] += w & 0xFFFFFFFFull;
    limb[(sh >> 5) + 1] += w >> 32;
}

void launch_docset_agg_ids(hipStream_t, const uint32_t* docs, uint32_t local_len, const DocsetAggD* aggs, uint32_t m, unsigned long long* state, uint32_t* mm, bool, uint32_t) {
    const char* k = "k_docset_agg_ids";
    agg_needs_host_loop(k);
    if (!local_len || !m) return;
    if (reinterpret_cast<uintptr_t>(docs) & 15u) agg_bad(k, "ids that are not 16-byte aligned");
    for (uint32_t i = 1; i < local_len; ++i)
        if (docs[i - 1] >= docs[i]) agg_bad(k, "ids that do not ascend");
    for (uint32_t i = local_len; i < ((local_len + 3u) & ~3u); ++i)
        if (docs[i] != 0xFFFFFFFFu) agg_bad(k, "ids without their padding");
    for (uint32_t f = 0; f < m; ++f) {
        const DocsetAggD& a = aggs[f];
        agg_check(k, a, state, mm);
        if (a.a_off || a.has_bits) agg_bad(k, "a 1:n column on the ids route");
        for (uint32_t i = 0; i < local_len; ++i) {
            const uint32_t row = docs[i] - a.key_base;
            if (docs[i] >= a.key_base && row < a.num_keys && (!a.present || agg_bit_of(a.present, row))) agg_add(a, a.values[row], state, mm);
            else ++state[a.state_off + kAggMissing];
        }
    }
}

void launch_docset_agg_values(hipStream_t, const DocsetAggD* aggs, uint32_t m, uint32_t max_keys, const uint32_t* member, uint32_t member_word0, uint32_t doc_lo,
                              uint32_t doc_hi, unsigned long long* state, uint32_t* mm, bool, uint32_t) {
    const char* k = "k_docset_agg_values";
    agg_needs_host_loop(k);
    if (!m) return;
    if (!member) agg_bad(k, "no membership bitmap");
    for (uint32_t f = 0; f < m; ++f) {
        const DocsetAggD& a = aggs[f];
        agg_check(k, a, state, mm);
        if (!a.a_off || !a.a_vals || !a.has_bits) agg_bad(k, "a 1:n column without its table or its has-a-value bitmap");
        if (reinterpret_cast<uintptr_t>(a.values) & 15u) agg_bad(k, "a column that is not 16-byte aligned");
        if (a.num_keys > max_keys) agg_bad(k, "a column longer than the grid was sized for");
        for (uint32_t r = 0; r < a.num_keys; ++r) {
            if (a.present && !agg_bit_of(a.present, r)) continue;
            const uint64_t vid = uint64_t(a.key_base) + r;
            if (vid < a.a_key_base || vid - a.a_key_base >= a.a_num_keys) continue;
            const uint64_t row = vid - a.a_key_base;
            if (a.a_off[row] > a.a_off[row + 1]) agg_bad(k, "CSR offsets that descend");
            if (a.a_off[row] == a.a_off[row + 1]) continue;
            const uint32_t anchor = a.a_vals[a.a_off[row]];
            if (anchor < doc_lo || anchor >= doc_hi) continue;
            if (!agg_bit_of(member, uint64_t(anchor) - uint64_t(member_word0) * 32)) continue;
            if (!agg_bit_of(a.has_bits, anchor)) {
                a.has_bits[anchor >> 5] |= 1u << (anchor & 31u);
                ++state[a.state_off + kAggHas];
            }
            agg_add(a, a.values[r], state, mm);
        }
    }
}
}  // namespace vq
