// TEST INFRASTRUCTURE — the launchers of veloci_amd/csrc/docset_ranges.hip for the host builds that stub the device layer (see hip_stub.cpp).
// Without VQ_STUB_DICT_SCAN they throw like every other launcher.  With VQ_STUB_DICT_SCAN=1 they are answered on the host by plain loops over the
// kernels' own operands — the clause descriptors with their key intervals, the columns and presence words, a within's bitmap words or padded ids,
// the value_id_to_anchor table — so that the host side of the doc sets from ranges (parsing, column resolution, the bounds' move to keys, the
// routing, the passes over a fixed clause table, the 1:n bitmaps, the shard sum, the error paths) runs end to end without a GPU.  What a kernel
// relies on and the host must guarantee is checked here and thrown when it does not hold.  Never linked into the product library.
#include <cstdlib>
#include <string>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
static void range_needs_host_loop(const char* what) {
    if (!std::getenv("VQ_STUB_DICT_SCAN")) throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: ") + what);
}
static void range_bad(const char* kernel, const char* what) { throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string(kernel) + " (stub): " + what); }
static bool range_bit_of(const uint32_t* words, uint64_t at) { return (words[at >> 5] >> (at & 31u)) & 1u; }
static void range_check_clause(const char* kernel, const RangeClauseD& c) {
    if (!c.values) range_bad(kernel, "a clause without a column");
    if (c.lo <= c.hi && (c.lo < kRangeKeyMin || c.hi > kRangeKeyMax)) range_bad(kernel, "an interval that reaches the NaNs");
}
// a column clause for one doc: apply_col_boost's addressing
static bool range_holds(const RangeClauseD& c, uint32_t doc) {
    const uint32_t row = doc - c.key_base;
    const bool present = doc >= c.key_base && row < c.num_keys && (!c.present || range_bit_of(c.present, row));
    if (!present) return c.missing != 0u;
    const uint32_t key = range_key(c.values[row]);
    return key >= c.lo && key <= c.hi;
}

void launch_range_bits(hipStream_t, const RangeClauseD* clauses, uint32_t n, const uint32_t* mask, uint32_t mask_word0, uint32_t* scratch, uint64_t scratch_words,
                       uint32_t doc_lo, uint32_t doc_hi) {
    const char* k = "k_range_bits";
    range_needs_host_loop(k);
    if (n > kRangeClauseTable) range_bad(k, "more clauses than the table holds");
    if (scratch_words % 16 || uint64_t(doc_hi) > scratch_words * 32) range_bad(k, "a doc range beyond the scratch bitmap");
    for (uint32_t i = 0; i < n; ++i) range_check_clause(k, clauses[i]);
    if (doc_hi <= doc_lo) return;
    for (uint64_t w = doc_lo >> 5; w < (uint64_t(doc_hi) + 31u) >> 5; ++w) {
        uint32_t word = 0;
        for (uint32_t bit = 0; bit < 32; ++bit) {
            const uint64_t doc = w * 32 + bit;
            if (doc < doc_lo || doc >= doc_hi) continue;
            bool ok = !mask || range_bit_of(mask, doc - uint64_t(mask_word0) * 32);
            for (uint32_t i = 0; i < n && ok; ++i) {
                const RangeClauseD& c = clauses[i];
                if (c.bitmap) ok = range_bit_of(c.values, doc) || (c.present && !range_bit_of(c.present, doc));
                else ok = range_holds(c, uint32_t(doc));
            }
            if (ok) word |= 1u << bit;
        }
        scratch[w] = word;
    }
}

void launch_range_probe(hipStream_t, const uint32_t* ids, uint32_t len, const RangeClauseD* clauses, uint32_t n, bool refine, uint32_t* scratch) {
    const char* k = "k_range_probe";
    range_needs_host_loop(k);
    if (n > kRangeClauseTable) range_bad(k, "more clauses than the table holds");
    if (reinterpret_cast<uintptr_t>(ids) & 15u) range_bad(k, "ids that are not 16-byte aligned");
    for (uint32_t i = 1; i < len; ++i)
        if (ids[i - 1] >= ids[i]) range_bad(k, "ids that do not ascend");
    for (uint32_t i = len; i < ((len + 3u) & ~3u); ++i)
        if (ids[i] != 0xFFFFFFFFu) range_bad(k, "ids without their padding");
    for (uint32_t i = 0; i < n; ++i) {
        range_check_clause(k, clauses[i]);
        if (clauses[i].bitmap) range_bad(k, "a 1:n clause on the probe route");
    }
    for (uint32_t i = 0; i < len; ++i) {
        bool keep = true;
        for (uint32_t c = 0; c < n && keep; ++c) keep = range_holds(clauses[c], ids[i]);
        if (!refine && keep) scratch[ids[i] >> 5] |= 1u << (ids[i] & 31u);
        if (refine && !keep) scratch[ids[i] >> 5] &= ~(1u << (ids[i] & 31u));
    }
}

void launch_range_scatter(hipStream_t, const RangeClauseD& column, const uint64_t* a_off, const uint32_t* a_vals, uint32_t a_key_base, uint32_t a_num_keys, uint32_t doc_lo,
                          uint32_t doc_hi, uint32_t* in_bits, uint32_t* has_bits) {
    const char* k = "k_range_scatter";
    range_needs_host_loop(k);
    range_check_clause(k, column);
    if (reinterpret_cast<uintptr_t>(column.values) & 15u) range_bad(k, "a column that is not 16-byte aligned");
    if (!in_bits || column.bitmap) range_bad(k, "no bitmap to fill, or a clause that is one already");
    for (uint32_t r = 0; r < column.num_keys; ++r) {
        if (column.present && !range_bit_of(column.present, r)) continue;
        const uint64_t vid = uint64_t(column.key_base) + r;
        if (vid < a_key_base || vid - a_key_base >= a_num_keys) continue;
        const uint64_t row = vid - a_key_base;
        if (a_off[row] > a_off[row + 1]) range_bad(k, "CSR offsets that descend");
        if (a_off[row] == a_off[row + 1]) continue;
        const uint32_t anchor = a_vals[a_off[row]];
        if (anchor < doc_lo || anchor >= doc_hi) continue;
        const uint32_t key = range_key(column.values[r]);
        if (key >= column.lo && key <= column.hi) in_bits[anchor >> 5] |= 1u << (anchor & 31u);
        if (has_bits) has_bits[anchor >> 5] |= 1u << (anchor & 31u);
    }
}
}  // namespace vq
