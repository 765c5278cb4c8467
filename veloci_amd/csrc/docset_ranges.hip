// Doc sets from numeric ranges: the docs whose column values lie in closed intervals, as one more way to fill the scratch bitmap over all anchors
// that docset.hip builds a set's image from (count -> scan -> expand -> tiles follow unchanged).  Plain kernels in sequence on one stream; one
// wave64 per workgroup, grids capped and strided; no workgroup waits for another.  Every kernel leaves bits inside [doc_lo, doc_hi) only (the host
// hands doc_hi cut to num_anchors), so the bitmap's popcount is the result's local length.
//
// A clause (RangeClauseD, kernels.hpp) is a dense f32 column with an optional presence bitmap — the image apply_col_boost reads: row = doc -
// key_base, no value when doc < key_base, row >= num_keys or the presence bit is clear — and a closed interval [lo, hi] of order-preserving keys
// (range_key: the sign-flipped bit pattern, -0 folded onto +0).  The host has cut the interval to [key(-inf), key(+inf)], so a NaN is present and
// outside every interval, and nothing here compares floats: the device's denormal mode has no say.  A doc without a value satisfies the clause
// when `missing` is set.  A kernel takes up to kRangeClauseTable clauses by value and a doc must satisfy all of them; the host
// (docset_ranges.cpp) runs longer lists in passes over the same scratch bitmap.
//
//   k_range_bits     the stream route.  A lane per doc: a wave takes kRangeUnroll groups of 64 docs (two scratch words each) per round, loads a
//                    clause's values and presence words of all its groups before it looks at any (8 + 8 independent loads per lane in flight),
//                    and the __ballot of "all clauses hold" is the group's two words.  `mask` (a within's bitmap image, or the scratch bitmap
//                    itself in a pass that and-s into what an earlier pass wrote) takes lanes out before the first load: a round whose docs are
//                    all masked loads nothing and writes nothing (its words are zero already).  Nothing depends on how key_base sits against a
//                    word or a vector.  A 1:n clause comes as the bitmaps k_range_scatter made, in the place of a column.
//   k_range_probe    the probe route, for a `within` without a bitmap.  Lanes stream its ids 16 B at a time and gather each id's value and
//                    presence word per clause (the four ids of a lane side by side).  The first pass ors the survivors into the zeroed scratch
//                    bitmap (no-return atomicOr), a later pass clears the ids that fail it.
//   k_range_scatter  a 1:n clause: the column is keyed by value id, a value belongs to the anchor in the first entry of its value_id_to_anchor
//                    row.  Lanes stream the column 16 B at a time; a present value inside the interval sets its anchor's bit in the clause's
//                    zeroed bitmap, and with `has_bits` every present value sets its anchor's bit there ("has a present value": the clause word
//                    is then in_range | ~has).  Anchors outside [doc_lo, doc_hi) and empty rows set nothing.
#include <algorithm>

#include "kernel_common.hpp"
#include "kernels.hpp"

namespace vq {

constexpr uint32_t kRangeMaxGrid = 8192;  // workgroups of one wave; the rest of the work is strided
constexpr uint32_t kRangeUnroll = 8;      // 64-doc groups a wave of k_range_bits holds at once

__device__ __forceinline__ bool range_bit(uint32_t word, uint32_t at) { return (word >> (at & 31u)) & 1u; }

// group0: the first 64-doc group (doc >> 6) the launch covers, n_groups of them: every group that touches [doc_lo, doc_hi).  mask: null, or words
// whose word (doc >> 5) - mask_word0 holds doc's bit; it may be `scratch` itself (a wave reads the words of its own groups only, before it writes them)
__global__ __launch_bounds__(64) void k_range_bits(const RangeClauseTable t, uint32_t n, const uint32_t* mask, uint32_t mask_word0, uint32_t* scratch, uint32_t group0,
                                                   uint32_t n_groups, uint32_t doc_lo, uint32_t doc_hi) {
    const uint32_t lane = lane_id();
    const uint32_t n_rounds = (n_groups + kRangeUnroll - 1u) / kRangeUnroll;
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {  // (uniform)
        const uint32_t g0 = round * kRangeUnroll;                              // groups [g0, g0 + kRangeUnroll) of the launch
        // (a doc of a group behind the last one may lie beyond 2^32: `in` is taken from the 64-bit id, the 32-bit one is used under it only)
        auto doc_of = [&](uint32_t u) { return ((unsigned long long)(group0 + g0 + u) << 6) + lane; };
        uint32_t alive = 0;  // bit u: this lane's doc of group g0 + u is inside the range and still holds
        uint32_t m[kRangeUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kRangeUnroll; ++u) {
            const unsigned long long d = doc_of(u);
            const bool in = g0 + u < n_groups && d >= doc_lo && d < doc_hi;
            m[u] = 0xFFFFFFFFu;
            if (in && mask) m[u] = as_global(mask)[((uint32_t)d >> 5) - mask_word0];
            if (in) alive |= 1u << u;
        }
#pragma unroll
        for (uint32_t u = 0; u < kRangeUnroll; ++u)
            if (!range_bit(m[u], (uint32_t)doc_of(u))) alive &= ~(1u << u);
        if (!__ballot(alive != 0u)) continue;  // (uniform) all masked: the words are zero already
        for (uint32_t k = 0; k < n; ++k) {     // (uniform trip count; the descriptors are wave-uniform)
            const uint32_t *values = t.c[k].values, *present = t.c[k].present;
            const uint32_t key_base = t.c[k].key_base, num_keys = t.c[k].num_keys, lo = t.c[k].lo, hi = t.c[k].hi;
            const bool missing = t.c[k].missing != 0u, is_bitmap = t.c[k].bitmap != 0u;
            uint32_t v[kRangeUnroll], p[kRangeUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kRangeUnroll; ++u) {
                const uint32_t doc = (uint32_t)doc_of(u), row = doc - key_base;
                const uint32_t at = is_bitmap ? doc >> 5 : row;
                const bool has = ((alive >> u) & 1u) && (is_bitmap || (doc >= key_base && row < num_keys));
                v[u] = 0u;
                p[u] = 0xFFFFFFFFu;
                if (has) v[u] = as_global(values)[at];
                if (has && present) p[u] = as_global(present)[is_bitmap ? at : at >> 5];
            }
#pragma unroll
            for (uint32_t u = 0; u < kRangeUnroll; ++u) {
                const uint32_t doc = (uint32_t)doc_of(u), row = doc - key_base;
                bool ok;
                if (is_bitmap) ok = range_bit(v[u], doc) || (present && !range_bit(p[u], doc));  // in_range | ~has
                else {
                    const bool pres = doc >= key_base && row < num_keys && range_bit(p[u], row);
                    const uint32_t key = range_key(v[u]);
                    ok = pres ? (key >= lo && key <= hi) : missing;
                }
                if (!ok) alive &= ~(1u << u);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kRangeUnroll; ++u) {
            const unsigned long long word = __ballot((alive >> u) & 1u);
            if (lane == 0 && g0 + u < n_groups) {
                uint32_t* out = scratch + ((unsigned long long)(group0 + g0 + u) << 1);
                out[0] = (uint32_t)word;
                out[1] = (uint32_t)(word >> 32);
            }
        }
    }
}

// ids: a set's sorted local ids, 16-byte aligned, padded to a multiple of 4 entries; every id lies inside the index's doc range.  Column clauses only
__global__ __launch_bounds__(64) void k_range_probe(const uint32_t* __restrict__ ids, uint32_t len, const RangeClauseTable t, uint32_t n, uint32_t refine,
                                                    uint32_t* __restrict__ bits) {
    const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(ids));
    const unsigned long long nvec = ((unsigned long long)len + 3u) >> 2;
    for (unsigned long long at = (unsigned long long)blockIdx.x * 64u + lane_id(); at < nvec; at += (unsigned long long)gridDim.x * 64u) {
        const u32x4 d = vec[at];
        const uint32_t id[4] = {d.x, d.y, d.z, d.w};
        uint32_t live = 0, keep;  // bit e: entry e is an id of the set / still holds
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e)
            if ((at << 2) + e < len) live |= 1u << e;
        keep = live;
        for (uint32_t k = 0; k < n; ++k) {  // (uniform trip count)
            const uint32_t *values = t.c[k].values, *present = t.c[k].present;
            const uint32_t key_base = t.c[k].key_base, num_keys = t.c[k].num_keys, lo = t.c[k].lo, hi = t.c[k].hi;
            const bool missing = t.c[k].missing != 0u;
            uint32_t v[4], p[4];
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) {
                const uint32_t row = id[e] - key_base;
                const bool has = ((keep >> e) & 1u) && id[e] >= key_base && row < num_keys;
                v[e] = 0u;
                p[e] = 0xFFFFFFFFu;
                if (has) v[e] = as_global(values)[row];
                if (has && present) p[e] = as_global(present)[row >> 5];
            }
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) {
                const uint32_t row = id[e] - key_base, key = range_key(v[e]);
                const bool pres = id[e] >= key_base && row < num_keys && range_bit(p[e], row);
                if (!(pres ? (key >= lo && key <= hi) : missing)) keep &= ~(1u << e);
            }
        }
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
            if (!((live >> e) & 1u)) continue;
            const bool kept = (keep >> e) & 1u;
            if (!refine && kept) atomicOr(bits + (id[e] >> 5), 1u << (id[e] & 31u));
            if (refine && !kept) atomicAnd(bits + (id[e] >> 5), ~(1u << (id[e] & 31u)));
        }
    }
}

// c: the column keyed by value id (16-byte aligned values with a vector of slack behind them) and the interval.  a_off / a_vals: the whole
// value_id_to_anchor table (row r = value id a_key_base + r).  in_bits / has_bits (null: not wanted): zeroed bitmaps of the scratch bitmap's shape
__global__ __launch_bounds__(64) void k_range_scatter(const RangeClauseD c, const unsigned long long* __restrict__ a_off, const uint32_t* __restrict__ a_vals,
                                                      uint32_t a_key_base, uint32_t a_num_keys, uint32_t doc_lo, uint32_t doc_hi, uint32_t* __restrict__ in_bits,
                                                      uint32_t* __restrict__ has_bits) {
    const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(c.values));
    const unsigned long long nvec = ((unsigned long long)c.num_keys + 3u) >> 2;
    for (unsigned long long at = (unsigned long long)blockIdx.x * 64u + lane_id(); at < nvec; at += (unsigned long long)gridDim.x * 64u) {
        const u32x4 d = vec[at];
        const uint32_t r0 = (uint32_t)(at << 2);  // (a multiple of 4: its four rows share a presence word)
        const uint32_t pw = c.present ? as_global(c.present)[r0 >> 5] : 0xFFFFFFFFu;
        const uint32_t val[4] = {d.x, d.y, d.z, d.w};
        uint32_t anchor[4], mark = 0;  // bit e: a present value with an anchor inside the shard; bit 4 + e: ... and inside the interval
        unsigned long long o0[4], o1[4];
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
            const uint32_t r = r0 + e, key = range_key(val[e]);
            const bool pres = r < c.num_keys && range_bit(pw, r), inside = pres && key >= c.lo && key <= c.hi;
            const unsigned long long vid = (unsigned long long)c.key_base + r, arow = vid - a_key_base;
            o0[e] = o1[e] = 0;
            if ((has_bits ? pres : inside) && vid >= a_key_base && arow < a_num_keys) {
                o0[e] = as_global(a_off)[arow];
                o1[e] = as_global(a_off)[arow + 1u];
                mark |= (1u | (inside ? 16u : 0u)) << e;
            }
        }
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
            if (o0[e] >= o1[e]) mark &= ~(17u << e);  // an empty row belongs to nobody
            anchor[e] = 0u;
            if ((mark >> e) & 1u) anchor[e] = as_global(a_vals)[o0[e]];
        }
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
            if (!((mark >> e) & 1u) || anchor[e] < doc_lo || anchor[e] >= doc_hi) continue;
            if ((mark >> (4u + e)) & 1u) atomicOr(in_bits + (anchor[e] >> 5), 1u << (anchor[e] & 31u));
            if (has_bits) atomicOr(has_bits + (anchor[e] >> 5), 1u << (anchor[e] & 31u));
        }
    }
}

static uint32_t range_grid(unsigned long long waves) { return (uint32_t)(waves < 1u ? 1u : waves < kRangeMaxGrid ? waves : kRangeMaxGrid); }
static RangeClauseTable range_table(const RangeClauseD* clauses, uint32_t n) {
    RangeClauseTable t{};
    for (uint32_t k = 0; k < n && k < kRangeClauseTable; ++k) t.c[k] = clauses[k];
    return t;
}

void launch_range_bits(hipStream_t st, const RangeClauseD* clauses, uint32_t n, const uint32_t* mask, uint32_t mask_word0, uint32_t* scratch, uint64_t scratch_words,
                       uint32_t doc_lo, uint32_t doc_hi) {
    if (n > kRangeClauseTable || doc_hi <= doc_lo) return;
    const uint64_t group0 = doc_lo >> 6, group_end = (uint64_t(doc_hi) + 63u) >> 6;
    if (group_end * 2u > scratch_words) return;  // (the scratch bitmap covers whole 512-doc blocks of all anchors)
    const uint32_t n_groups = uint32_t(group_end - group0);
    hipLaunchKernelGGL(k_range_bits, dim3(range_grid((n_groups + kRangeUnroll - 1u) / kRangeUnroll)), dim3(64), 0, st, range_table(clauses, n), n, mask, mask_word0, scratch,
                       uint32_t(group0), n_groups, doc_lo, doc_hi);
}
void launch_range_probe(hipStream_t st, const uint32_t* ids, uint32_t len, const RangeClauseD* clauses, uint32_t n, bool refine, uint32_t* scratch) {
    if (!len || n > kRangeClauseTable) return;
    hipLaunchKernelGGL(k_range_probe, dim3(range_grid((len / 4u + 63u) / 64u)), dim3(64), 0, st, ids, len, range_table(clauses, n), n, refine ? 1u : 0u, scratch);
}
void launch_range_scatter(hipStream_t st, const RangeClauseD& column, const uint64_t* a_off, const uint32_t* a_vals, uint32_t a_key_base, uint32_t a_num_keys, uint32_t doc_lo,
                          uint32_t doc_hi, uint32_t* in_bits, uint32_t* has_bits) {
    if (!column.num_keys || !a_num_keys || doc_hi <= doc_lo) return;
    hipLaunchKernelGGL(k_range_scatter, dim3(range_grid((column.num_keys / 4u + 63u) / 64u)), dim3(64), 0, st, column, reinterpret_cast<const unsigned long long*>(a_off), a_vals,
                       a_key_base, a_num_keys, doc_lo, doc_hi, in_bits, has_bits);
}

}  // namespace vq
