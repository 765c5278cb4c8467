// Doc set algebra: and / or / minus / complement of staged sets, as one more way to fill the scratch bitmap over all anchors that docset.hip builds a
// set's image from (count -> scan -> expand -> tiles follow unchanged).  Plain kernels in sequence on one stream; one wave64 per workgroup, grids
// capped and strided; no workgroup waits for another; 16 B per lane in the inner loops.  Every kernel leaves bits inside [doc_lo, doc_hi) and below
// num_anchors only, so the bitmap's popcount is the result's local length.
//
// An operand (SetOperand, kernels.hpp) is a set's bitmap image where it carries one (word j = docs [bitmap_base + 32 j, + 32), the same base and
// word count for every set of an index: scratch word base_word + j) and its sorted local ids (padded to a multiple of 4 with 0xFFFFFFFF).  A kernel
// takes up to kSetOpTable operands by value; the host (docset_algebra.cpp) runs longer lists in rounds over the same scratch bitmap.
//
//   k_setop_words   the word route.  Lanes walk the local image 16 B at a time and fold the operands' bitmap words into the scratch bitmap:
//                     or      scratch | o[0] | o[1] | ...
//                     else    start & o[0] & ... & o[n_pos - 1] & ~(o[n_pos] | ... | o[n - 1]), masked to [doc_lo, doc_hi);  start = all ones in the
//                             first round, the scratch words in a later one.  and: n_pos = n.  minus: the minuend is o[0] of the first round,
//                             n_pos = 0 afterwards.  not: n_pos = 0, n = 1, all ones.
//   k_setop_clear   a bitmap-less subtrahend (or the operand of not): lanes stream its ids 16 B at a time and atomicAnd the inverted bit.
//   k_setop_probe   the probe route, for results bounded by a sparse operand.  Lanes stream the leader's ids 16 B at a time and test each against
//                   every other operand: one bit test in a bitmap, a binary search in sorted ids.  and: an id survives when all hold it, minus: when
//                   none does.  The first round ors the survivors into the zeroed scratch bitmap, a later round clears the ids that fail it.
#include <algorithm>

#include "kernel_common.hpp"
#include "kernels.hpp"

namespace vq {

constexpr uint32_t kSetOpMaxGrid = 8192;  // workgroups of one wave; the rest of the work is strided

// the bits of local word j that lie inside [lo, hi)
__device__ __forceinline__ uint32_t setop_range_mask(unsigned long long j, uint32_t bitmap_base, uint32_t lo, uint32_t hi) {
    const unsigned long long doc0 = (unsigned long long)bitmap_base + (j << 5);
    if (doc0 + 32u <= lo || doc0 >= hi) return 0u;
    uint32_t m = 0xFFFFFFFFu;
    if (doc0 < lo) m &= 0xFFFFFFFFu << (uint32_t)(lo - doc0);
    if (doc0 + 32u > hi) m &= (1u << (uint32_t)(hi - doc0)) - 1u;
    return m;
}

// local: scratch + base_word; nvec: 16-byte vectors of the local image that lie inside the scratch bitmap
__global__ __launch_bounds__(64) void k_setop_words(const SetOpTable t, uint32_t n_pos, uint32_t n, uint32_t is_or, uint32_t init_ones, uint32_t* local,
                                                    unsigned long long nvec, uint32_t bitmap_base, uint32_t doc_lo, uint32_t doc_hi) {
    u32x4* out = reinterpret_cast<u32x4*>(local);
    for (unsigned long long v = (unsigned long long)blockIdx.x * 64u + lane_id(); v < nvec; v += (unsigned long long)gridDim.x * 64u) {
        u32x4 acc = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (!init_ones) acc = as_global(reinterpret_cast<const u32x4*>(local))[v];  // (uniform; this lane alone reads and writes vector v)
        if (is_or) {
            for (uint32_t k = 0; k < n; ++k) acc |= as_global(reinterpret_cast<const u32x4*>(t.o[k].bitmap))[v];  // (uniform trip count)
        } else {
            for (uint32_t k = 0; k < n_pos; ++k) acc &= as_global(reinterpret_cast<const u32x4*>(t.o[k].bitmap))[v];
            u32x4 neg = u32x4{0u, 0u, 0u, 0u};
            for (uint32_t k = n_pos; k < n; ++k) neg |= as_global(reinterpret_cast<const u32x4*>(t.o[k].bitmap))[v];
            acc &= ~neg;
            const unsigned long long j = v << 2;
            acc &= u32x4{setop_range_mask(j, bitmap_base, doc_lo, doc_hi), setop_range_mask(j + 1u, bitmap_base, doc_lo, doc_hi),
                         setop_range_mask(j + 2u, bitmap_base, doc_lo, doc_hi), setop_range_mask(j + 3u, bitmap_base, doc_lo, doc_hi)};
        }
        out[v] = acc;
    }
}

// ids: sorted ids below num_anchors, 16-byte aligned, padded to a multiple of 4 entries
__global__ __launch_bounds__(64) void k_setop_clear(const uint32_t* __restrict__ ids, uint32_t n, uint32_t* __restrict__ bits) {
    const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(ids));
    const unsigned long long nvec = ((unsigned long long)n + 3u) >> 2;
    for (unsigned long long v = (unsigned long long)blockIdx.x * 64u + lane_id(); v < nvec; v += (unsigned long long)gridDim.x * 64u) {
        const u32x4 d = vec[v];
        const unsigned long long at = v << 2;
        if (at < n) atomicAnd(bits + (d.x >> 5), ~(1u << (d.x & 31u)));
        if (at + 1u < n) atomicAnd(bits + (d.y >> 5), ~(1u << (d.y & 31u)));
        if (at + 2u < n) atomicAnd(bits + (d.z >> 5), ~(1u << (d.z & 31u)));
        if (at + 3u < n) atomicAnd(bits + (d.w >> 5), ~(1u << (d.w & 31u)));
    }
}

// is `id` among a[0 .. n) (ascending)?
__device__ __forceinline__ bool setop_holds(const uint32_t* __restrict__ a_, uint32_t n, uint32_t id) {
    const VQ_GLOBAL uint32_t* a = as_global(a_);
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < id) lo = mid + 1u;
        else hi = mid;
    }
    return lo < n && a[lo] == id;
}

// leader: as the ids of k_setop_clear, every id inside [doc_lo, doc_hi).  negate: an id survives when no operand holds it (else: when all do)
__global__ __launch_bounds__(64) void k_setop_probe(const uint32_t* __restrict__ leader, uint32_t leader_len, const SetOpTable t, uint32_t n, uint32_t negate, uint32_t refine,
                                                    uint32_t bitmap_base, uint32_t* __restrict__ bits) {
    const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(leader));
    const unsigned long long nvec = ((unsigned long long)leader_len + 3u) >> 2;
    for (unsigned long long v = (unsigned long long)blockIdx.x * 64u + lane_id(); v < nvec; v += (unsigned long long)gridDim.x * 64u) {
        const u32x4 d = vec[v];
        const unsigned long long at = v << 2;
        auto test = [&](uint32_t id, bool live) {
            if (!live) return;
            bool keep = true;
            for (uint32_t k = 0; k < n && keep; ++k) {
                bool in;
                if (t.o[k].bitmap) {
                    const uint32_t rel = id - bitmap_base;
                    in = (as_global(t.o[k].bitmap)[rel >> 5] >> (rel & 31u)) & 1u;
                } else in = setop_holds(t.o[k].docs, t.o[k].len, id);
                keep = in != (negate != 0u);
            }
            if (!refine && keep) atomicOr(bits + (id >> 5), 1u << (id & 31u));
            if (refine && !keep) atomicAnd(bits + (id >> 5), ~(1u << (id & 31u)));
        };
        test(d.x, at < leader_len);
        test(d.y, at + 1u < leader_len);
        test(d.z, at + 2u < leader_len);
        test(d.w, at + 3u < leader_len);
    }
}

static uint32_t setop_grid(unsigned long long waves) { return (uint32_t)(waves < 1u ? 1u : waves < kSetOpMaxGrid ? waves : kSetOpMaxGrid); }
static SetOpTable setop_table(const SetOperand* ops, uint32_t n) {
    SetOpTable t{};
    for (uint32_t k = 0; k < n && k < kSetOpTable; ++k) t.o[k] = ops[k];
    return t;
}

void launch_setop_words(hipStream_t st, const SetOperand* ops, uint32_t n_pos, uint32_t n, bool is_or, bool init_ones, uint32_t* scratch, uint64_t scratch_words, uint64_t base_word,
                        uint64_t words, uint32_t bitmap_base, uint32_t doc_lo, uint32_t doc_hi) {
    if (n > kSetOpTable || n_pos > n || base_word >= scratch_words) return;
    const uint64_t nvec = std::min(words, scratch_words - base_word) >> 2;  // (both are multiples of 16 words)
    if (!nvec) return;
    hipLaunchKernelGGL(k_setop_words, dim3(setop_grid((nvec + 63u) / 64u)), dim3(64), 0, st, setop_table(ops, n), n_pos, n, is_or ? 1u : 0u, init_ones ? 1u : 0u, scratch + base_word,
                       (unsigned long long)nvec, bitmap_base, doc_lo, doc_hi);
}
void launch_setop_clear(hipStream_t st, const uint32_t* ids, uint32_t n, uint32_t* scratch) {
    if (!n) return;
    hipLaunchKernelGGL(k_setop_clear, dim3(setop_grid((n / 4u + 63u) / 64u)), dim3(64), 0, st, ids, n, scratch);
}
void launch_setop_probe(hipStream_t st, const uint32_t* leader, uint32_t leader_len, const SetOperand* ops, uint32_t n, bool negate, bool refine, uint32_t bitmap_base,
                        uint32_t* scratch) {
    if (!leader_len || n > kSetOpTable) return;
    hipLaunchKernelGGL(k_setop_probe, dim3(setop_grid((leader_len / 4u + 63u) / 64u)), dim3(64), 0, st, leader, leader_len, setop_table(ops, n), n, negate ? 1u : 0u, refine ? 1u : 0u,
                       bitmap_base, scratch);
}

}  // namespace vq
