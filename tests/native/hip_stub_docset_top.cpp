// TEST INFRASTRUCTURE — the launchers of veloci_amd/csrc/docset_top.hip for the host builds that stub the device layer (see hip_stub.cpp).
// Without VQ_STUB_DICT_SCAN they throw like every other launcher.  With VQ_STUB_DICT_SCAN=1 they are answered on the host by plain loops over the
// kernels' own operands — the descriptor, the column and presence words, the set's padded ids, the membership bitmap, the value_id_to_anchor
// table — into the kernels' own state layout (kernels.hpp: keys, four histograms, chunk counts, state words, output pairs), so that the host side
// of a doc set ordered by a column (spec parsing, column resolution, the scratch area, the kernel sequence, the final order, skip and top, the
// shard parts with merge, pack and unpack, the error paths) runs end to end without a GPU.  The emit writes the rows below the threshold in
// REVERSE order: the device hands those slots out in no order, and the host must not rely on one.  What a kernel relies on and the host must
// guarantee is checked here and thrown when it does not hold.  Never linked into the product library.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
static void top_needs_host_loop(const char* what) {
    if (!std::getenv("VQ_STUB_DICT_SCAN")) throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: ") + what);
}
static void top_bad(const char* kernel, const char* what) { throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string(kernel) + " (stub): " + what); }
static bool top_bit_of(const uint32_t* words, uint64_t at) { return (words[at >> 5] >> (at & 31u)) & 1u; }
static uint32_t top_key_of(uint32_t bits, uint32_t descending) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return kTopNanKey;
    return descending ? ~range_key(bits) : range_key(bits);
}
static uint64_t top_vectors(uint32_t n) { return (uint64_t(n) + 3u) / 4u; }
static void top_check_state(const char* k, const uint32_t* state) {
    if (reinterpret_cast<uintptr_t>(state) & 3u) top_bad(k, "a state area that is not aligned");
    if (state[kTopDone] > 1u || state[kTopAllTies] > 1u) top_bad(k, "flags that are no flags");
}

void launch_top_fold(hipStream_t, const DocsetTopD& a, const uint32_t* member, uint32_t member_word0, uint32_t doc_hi, uint32_t* best, uint32_t) {
    const char* k = "k_top_fold";
    top_needs_host_loop(k);
    if (!a.num_keys || doc_hi <= a.doc_lo) return;
    if (!member || !best) top_bad(k, "no membership bitmap or no fold array");
    if (!a.values || !a.a_off || !a.a_vals) top_bad(k, "a 1:n column without its table");
    if (reinterpret_cast<uintptr_t>(a.values) & 15u) top_bad(k, "a column that is not 16-byte aligned");
    for (uint32_t d = a.doc_lo; d < doc_hi; ++d)
        if (best[d - a.doc_lo] != kTopMissingKey) top_bad(k, "a fold array that is not preset to the missing key");
    for (uint32_t r = 0; r < a.num_keys; ++r) {
        if (a.present && !top_bit_of(a.present, r)) continue;
        const uint64_t vid = uint64_t(a.key_base) + r;
        if (vid < a.a_key_base || vid - a.a_key_base >= a.a_num_keys) continue;
        const uint64_t row = vid - a.a_key_base;
        if (a.a_off[row] > a.a_off[row + 1]) top_bad(k, "CSR offsets that descend");
        if (a.a_off[row] == a.a_off[row + 1]) continue;
        const uint32_t anchor = a.a_vals[a.a_off[row]];
        if (anchor < a.doc_lo || anchor >= doc_hi) continue;
        if (!top_bit_of(member, uint64_t(anchor) - uint64_t(member_word0) * 32)) continue;
        const uint32_t key = top_key_of(a.values[r], a.descending);
        if (key < best[anchor - a.doc_lo]) best[anchor - a.doc_lo] = key;
    }
}

void launch_top_keys(hipStream_t, const uint32_t* docs, uint32_t local_len, const DocsetTopD& a, uint32_t* keys, uint32_t* hist, uint32_t* state, uint32_t) {
    const char* k = "k_top_keys";
    top_needs_host_loop(k);
    if (!local_len) return;
    top_check_state(k, state);
    if ((reinterpret_cast<uintptr_t>(docs) & 15u) || (reinterpret_cast<uintptr_t>(keys) & 15u)) top_bad(k, "ids or keys that are not 16-byte aligned");
    for (uint32_t i = 1; i < local_len; ++i)
        if (docs[i - 1] >= docs[i]) top_bad(k, "ids that do not ascend");
    for (uint32_t i = local_len; i < ((local_len + 3u) & ~3u); ++i)
        if (docs[i] != 0xFFFFFFFFu) top_bad(k, "ids without their padding");
    if (state[kTopCount] || state[kTopNan] || state[kTopMissing] || state[kTopCursor]) top_bad(k, "counters that are not zeroed");
    for (uint32_t i = 0; i < 4u * 256u; ++i)
        if (hist[i]) top_bad(k, "histograms that are not zeroed");
    if (!a.best && !a.values) top_bad(k, "no column");
    if (a.best && docs[0] < a.doc_lo) top_bad(k, "an id below the fold array");
    for (uint32_t i = 0; i < local_len; ++i) {
        uint32_t key = kTopMissingKey;
        if (a.best) {
            key = a.best[docs[i] - a.doc_lo];
        } else {
            const uint32_t row = docs[i] - a.key_base;
            if (docs[i] >= a.key_base && row < a.num_keys && (!a.present || top_bit_of(a.present, row))) key = top_key_of(a.values[row], a.descending);
        }
        keys[i] = key;
        ++hist[key >> 24];
        ++state[key <= kRangeKeyMax ? kTopCount : key == kTopNanKey ? kTopNan : kTopMissing];
        if (key < kRangeKeyMin || (key > kRangeKeyMax && key < kTopNanKey)) top_bad(k, "a sort key that no value has");
    }
    for (uint32_t i = local_len; i < ((local_len + 3u) & ~3u); ++i) keys[i] = kTopMissingKey;
}

void launch_top_pick(hipStream_t, uint32_t* state, const uint32_t* hist, uint32_t shift, uint32_t rows, bool with_missing, uint32_t n) {
    const char* k = "k_top_pick";
    top_needs_host_loop(k);
    top_check_state(k, state);
    if (shift != 24u && shift != 16u && shift != 8u && shift != 0u) top_bad(k, "a shift that is no byte of the key");
    if (rows > kTopMaxRows) top_bad(k, "more rows than a call may ask for");
    if (state[kTopDone]) return;
    uint32_t want = state[kTopWant], prefix = state[kTopPrefix], below = state[kTopB];
    uint64_t total = 0;
    for (uint32_t b = 0; b < 256u; ++b) total += hist[b];
    if (shift == 24u) {
        const uint32_t eligible = with_missing ? n : state[kTopCount];
        if (total != n) top_bad(k, "a first histogram that does not hold every key");
        want = rows < eligible ? rows : eligible;
        prefix = 0;
        below = 0;
    }
    if (want > total) top_bad(k, "more rows wanted than the histogram holds");
    if (!want) {
        state[kTopT] = state[kTopB] = state[kTopE] = state[kTopTake] = state[kTopAllTies] = state[kTopWant] = 0u;
        state[kTopDone] = 1u;
        return;
    }
    uint32_t seen = 0, bin = 0;
    while (seen + hist[bin] < want) seen += hist[bin++];
    prefix |= bin << shift;
    state[kTopPrefix] = prefix;
    state[kTopWant] = want - seen;
    state[kTopB] = below + seen;
    if (shift == 0u) {
        state[kTopT] = prefix;
        state[kTopE] = hist[bin];
        state[kTopTake] = want - seen;
        state[kTopAllTies] = hist[bin] == want - seen ? 1u : 0u;
    }
}

void launch_top_hist(hipStream_t, const uint32_t* keys, uint32_t n, uint32_t shift, const uint32_t* state, uint32_t* hist, uint32_t) {
    const char* k = "k_top_hist";
    top_needs_host_loop(k);
    if (!n || shift > 16u) return;
    top_check_state(k, state);
    if (reinterpret_cast<uintptr_t>(keys) & 15u) top_bad(k, "keys that are not 16-byte aligned");
    if (state[kTopDone]) return;
    for (uint32_t b = 0; b < 256u; ++b)
        if (hist[b]) top_bad(k, "a histogram that is not zeroed");
    const uint32_t prefix = state[kTopPrefix], mask = 0xFFFFFFFFu << (shift + 8u);
    if (prefix & ~mask) top_bad(k, "a prefix with digits that were not agreed yet");
    for (uint32_t i = 0; i < n; ++i)
        if ((keys[i] & mask) == prefix) ++hist[(keys[i] >> shift) & 0xFFu];
}

void launch_top_tiecount(hipStream_t, const uint32_t* keys, uint32_t n, const uint32_t* state, uint32_t* chunks, uint32_t max_grid) {
    const char* k = "k_top_tiecount";
    top_needs_host_loop(k);
    if (!n) return;
    top_check_state(k, state);
    if (state[kTopDone] || state[kTopAllTies] || !state[kTopTake]) return;
    const uint64_t nvec = top_vectors(n);
    const uint32_t grid = top_grid(nvec, max_grid);
    if (!grid || grid > kTopMaxGrid) top_bad(k, "a grid the chunk counts do not hold");
    const uint64_t vpc = (nvec + grid - 1u) / grid;
    for (uint32_t c = 0; c < grid; ++c) {
        uint32_t mine = 0;
        for (uint64_t i = uint64_t(c) * vpc * 4u; i < std::min<uint64_t>(n, (uint64_t(c) + 1u) * vpc * 4u); ++i) mine += keys[i] == state[kTopT];
        chunks[c] = mine;
    }
}

void launch_top_emit(hipStream_t, const uint32_t* docs, const uint32_t* keys, uint32_t n, uint32_t* state, const uint32_t* chunks, unsigned long long* out, uint32_t cap,
                     uint32_t max_grid) {
    const char* k = "k_top_emit";
    top_needs_host_loop(k);
    if (!n || !cap) return;
    top_check_state(k, state);
    if (reinterpret_cast<uintptr_t>(out) & 7u) top_bad(k, "output pairs that are not aligned");
    if (state[kTopDone]) return;
    const uint32_t T = state[kTopT], B = state[kTopB], all = state[kTopAllTies], take = all ? 0u : state[kTopTake];
    if (state[kTopCursor]) top_bad(k, "a cursor that is not zeroed");
    uint64_t low = 0;
    for (uint32_t i = 0; i < n; ++i) low += keys[i] < T || (all && keys[i] == T);
    if (low > cap || uint64_t(B) + take > cap) top_bad(k, "more rows than the output holds");
    if (!all && low != B) top_bad(k, "B is not the number of keys below the threshold");
    uint64_t at = low;  // the rows through the cursor: in reverse, the device keeps no order among them
    for (uint32_t i = 0; i < n; ++i)
        if (keys[i] < T || (all && keys[i] == T)) out[--at] = (uint64_t(keys[i]) << 32) | docs[i];
    state[kTopCursor] = uint32_t(low);
    if (take) {  // the ties by chunk offset + rank inside the chunk, as the kernel ranks them
        const uint64_t nvec = top_vectors(n);
        const uint32_t grid = top_grid(nvec, max_grid);
        const uint64_t vpc = (nvec + grid - 1u) / grid;
        uint32_t before = 0;
        for (uint32_t c = 0; c < grid; ++c) {
            uint32_t rank = before;
            for (uint64_t i = uint64_t(c) * vpc * 4u; i < std::min<uint64_t>(n, (uint64_t(c) + 1u) * vpc * 4u); ++i)
                if (keys[i] == T) {
                    if (rank < take) out[B + rank] = (uint64_t(keys[i]) << 32) | docs[i];
                    ++rank;
                }
            if (rank - before != chunks[c]) top_bad(k, "a chunk count that is not the chunk's ties");
            before = rank;
        }
        if (before != state[kTopE]) top_bad(k, "E is not the number of keys equal to the threshold");
    }
}
}  // namespace vq
