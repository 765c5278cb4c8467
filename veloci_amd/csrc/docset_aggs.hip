// Numeric aggregations of a doc set: count, missing, NaN count, min, max, an exact sum and range-bucket counts of f32 columns over a staged set's
// docs (DocsetAggD and the state layout: kernels.hpp).  Plain kernels on one stream; one wave64 per workgroup, grids capped and strided; no
// workgroup waits for another; plain loads, vector stores and integer atomics only — no float is added or compared anywhere, so the device's
// denormal mode and the order of the atomics have no say: every number is an integer, the sum is a fixed-point integer of 9 x 32 bits per sign
// that the host rounds once (docset_aggs.cpp: agg_limbs_to_double).
//
//   k_docset_agg_ids     anchor-keyed columns, grid (x, m): workgroup (x, f) aggregates aggs[f] over its stride of the set's ids.  Lanes stream
//                        DocSet::docs 16 B at a time (four ids per lane and round, bounded by local_len: the padding is never counted), gather the
//                        four values and presence words together, then accumulate: counters and the min / max key in registers (folded into LDS
//                        once per lane at the end: atomicAdd / atomicMin / atomicMax), the bucket histogram in LDS (u32; the edge keys in LDS,
//                        upper-bound binary search), the sum's limbs in LDS (u64).  Non-zero state is flushed to HBM once, at the end of the
//                        stride: u64 atomicAdd for counters, buckets and limbs, u32 atomicMin / atomicMax for the keys.  Cost follows the set.
//   k_docset_agg_values  1:n columns, grid (x, m): lanes stream the value column 16 B at a time like k_range_scatter; a present value looks up its
//                        anchor (the first entry of its value_id_to_anchor row) and tests it against the membership bitmap (the set's own
//                        bitmap image, or the scratch bitmap launch_docset_mark filled).  The lane whose returning atomicOr finds the anchor's
//                        bit of the zeroed has-a-value bitmap clear counts the doc once (kAggHas).
//
// The sum: values of one column tend to share an exponent, so their addends land on one or two limbs and LDS atomics on them serialise.  With
// kPre the addends of a round are summed per limb across the wave first (four 16-bit pieces through the DPP add-scan, all integer) and lane 0
// adds the totals with a plain read-modify-write (the LDS belongs to the one wave); without it every value issues its two LDS atomics.
#include <algorithm>

#include "kernel_common.hpp"
#include "kernels.hpp"

namespace vq {

constexpr uint32_t kAggMaxGrid = 2048;  // workgroups of one wave per aggregation; the rest of the work is strided
constexpr uint32_t kAggNoSlot = 0xFFu;

struct AggLds {
    uint32_t* edges;           // [kAggMaxEdges + 1]
    uint32_t* hist;            // [kAggMaxEdges + 1]
    unsigned long long* limb;  // [2 * kAggLimbsPerSign]
    uint32_t* cnt;             // [8]: the state's five counters, then the min key and the max key
};
struct AggLane {  // what a lane keeps in registers over its stride
    uint32_t count = 0, other = 0, nan = 0, pinf = 0, ninf = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
};

__device__ __forceinline__ bool agg_bit(uint32_t word, uint32_t at) { return (word >> (at & 31u)) & 1u; }

// one present value: counters, keys and bucket; -> the limb slot its addend *w goes to, or kAggNoSlot (NaN, infinity, zero)
__device__ __forceinline__ uint32_t agg_value(uint32_t bits, uint32_t n_edges, const AggLds& s, AggLane& l, unsigned long long* w) {
    const uint32_t mag = bits & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) {
        ++l.nan;
        return kAggNoSlot;
    }
    ++l.count;
    const uint32_t key = range_key(bits);
    l.kmin = key < l.kmin ? key : l.kmin;
    l.kmax = key > l.kmax ? key : l.kmax;
    if (n_edges) {  // (uniform) the number of edge keys <= key
        uint32_t lo = 0, hi = n_edges;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s.edges[mid] <= key) lo = mid + 1u;
            else hi = mid;
        }
        atomicAdd(&s.hist[lo], 1u);
    }
    if (mag == 0x7F800000u) {
        if (bits >> 31) ++l.ninf;
        else ++l.pinf;
        return kAggNoSlot;
    }
    if (mag == 0u) return kAggNoSlot;
    const uint32_t be = mag >> 23, m = be ? ((mag & 0x007FFFFFu) | 0x00800000u) : mag, sh = (be ? be : 1u) - 1u;
    *w = (unsigned long long)m << (sh & 31u);
    return (bits >> 31) * kAggLimbsPerSign + (sh >> 5);
}

// the four addends of every lane (slot[e] == kAggNoSlot: none) into the limbs.  All lanes of the wave call this together
template <bool kPre>
__device__ __forceinline__ void agg_sum(const AggLds& s, const uint32_t (&slot)[4], const unsigned long long (&w)[4]) {
    if (!kPre) {
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e)
            if (slot[e] != kAggNoSlot) {
                atomicAdd(&s.limb[slot[e]], w[e] & 0xFFFFFFFFull);
                if (w[e] >> 32) atomicAdd(&s.limb[slot[e] + 1u], w[e] >> 32);
            }
        return;
    }
    const uint32_t slots = slot[0] | (slot[1] << 8) | (slot[2] << 16) | (slot[3] << 24);
    uint32_t pend = 0;
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e)
        if (slot[e] != kAggNoSlot) pend |= 1u << e;
    for (;;) {
        const unsigned long long any = __ballot(pend != 0u);
        if (!any) break;  // (uniform)
        const uint32_t src = (uint32_t)__ffsll((long long)any) - 1u;
        const uint32_t mine = pend ? (slots >> (8u * ((uint32_t)__ffs((int)pend) - 1u))) & 0xFFu : 0u;
        const uint32_t cur = (uint32_t)__shfl((int)mine, (int)src);  // (uniform) the slot this round adds up
        uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;  // 16-bit pieces of this lane's addends: a wave's total of each stays below 2^26
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e)
            if (((pend >> e) & 1u) && slot[e] == cur) {
                p0 += (uint32_t)w[e] & 0xFFFFu;
                p1 += (uint32_t)(w[e] >> 16) & 0xFFFFu;
                p2 += (uint32_t)(w[e] >> 32) & 0xFFFFu;
                p3 += (uint32_t)(w[e] >> 48);
                pend &= ~(1u << e);
            }
        uint32_t t0, t1, t2, t3;
        wave_excl_scan_u32(p0, &t0);
        wave_excl_scan_u32(p1, &t1);
        wave_excl_scan_u32(p2, &t2);
        wave_excl_scan_u32(p3, &t3);
        if (lane_id() == 0u) {  // (the LDS is this wave's alone; nobody else touches the limbs in this mode)
            s.limb[cur] += (unsigned long long)t0 + ((unsigned long long)t1 << 16);
            s.limb[cur + 1u] += (unsigned long long)t2 + ((unsigned long long)t3 << 16);
        }
    }
}

__device__ __forceinline__ void agg_init(const AggLds& s, const DocsetAggD& a) {
    const uint32_t lane = lane_id();
    for (uint32_t i = lane; i <= a.n_edges; i += 64u) {
        s.hist[i] = 0u;
        if (i < a.n_edges) s.edges[i] = as_global(a.edges)[i];
    }
    if (lane < 2u * kAggLimbsPerSign) s.limb[lane] = 0ull;
    if (lane < 8u) s.cnt[lane] = lane == 5u ? 0xFFFFFFFFu : 0u;
    __syncthreads();
}

// the lanes' registers into LDS, then the workgroup's non-zero state into HBM
__device__ __forceinline__ void agg_flush(const AggLds& s, const DocsetAggD& a, const AggLane& l, unsigned long long* __restrict__ state, uint32_t* __restrict__ mm) {
    const uint32_t lane = lane_id();
    if (l.count) atomicAdd(&s.cnt[kAggCount], l.count);
    if (l.other) atomicAdd(&s.cnt[kAggMissing], l.other);
    if (l.nan) atomicAdd(&s.cnt[kAggNan], l.nan);
    if (l.pinf) atomicAdd(&s.cnt[kAggPosInf], l.pinf);
    if (l.ninf) atomicAdd(&s.cnt[kAggNegInf], l.ninf);
    if (l.count) {
        atomicMin(&s.cnt[5], l.kmin);
        atomicMax(&s.cnt[6], l.kmax);
    }
    __syncthreads();
    unsigned long long* out = state + a.state_off;
    if (lane < kAggLimbs && s.cnt[lane]) atomicAdd(&out[lane], (unsigned long long)s.cnt[lane]);
    if (lane < 2u * kAggLimbsPerSign && s.limb[lane]) atomicAdd(&out[kAggLimbs + lane], s.limb[lane]);
    if (a.n_edges)
        for (uint32_t i = lane; i <= a.n_edges; i += 64u)
            if (s.hist[i]) atomicAdd(&out[kAggBuckets + i], (unsigned long long)s.hist[i]);
    if (lane == 0u && s.cnt[kAggCount]) {
        atomicMin(&mm[a.mm_off], s.cnt[5]);
        atomicMax(&mm[a.mm_off + 1u], s.cnt[6]);
    }
}

#define VQ_AGG_LDS                                                      \
    __shared__ uint32_t lds_edges[kAggMaxEdges + 1u];                   \
    __shared__ uint32_t lds_hist[kAggMaxEdges + 1u];                    \
    __shared__ unsigned long long lds_limb[2u * kAggLimbsPerSign];      \
    __shared__ uint32_t lds_cnt[8];                                     \
    const AggLds s{lds_edges, lds_hist, lds_limb, lds_cnt}

// docs: 16-byte aligned, (local_len + 3) / 4 whole vectors; state zeroed, mm = {0xFFFFFFFF, 0} per aggregation before the launch
template <bool kPre>
__global__ __launch_bounds__(64) void k_docset_agg_ids(const uint32_t* __restrict__ docs, uint32_t local_len, const DocsetAggD* __restrict__ aggs,
                                                       unsigned long long* __restrict__ state, uint32_t* __restrict__ mm) {
    VQ_AGG_LDS;
    const uint32_t lane = lane_id();
    const DocsetAggD a = aggs[blockIdx.y];  // (uniform)
    agg_init(s, a);
    AggLane l;
    const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(docs));
    const unsigned long long nvec = ((unsigned long long)local_len + 3u) >> 2;
    for (unsigned long long v0 = (unsigned long long)blockIdx.x * 64u; v0 < nvec; v0 += (unsigned long long)gridDim.x * 64u) {  // (uniform trip count)
        const unsigned long long v = v0 + lane;
        u32x4 d = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (v < nvec) d = vec[v];
        const uint32_t id[4] = {d.x, d.y, d.z, d.w};
        uint32_t val[4], pw[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const uint32_t row = id[e] - a.key_base;
            const bool has = (v << 2) + e < local_len && id[e] >= a.key_base && row < a.num_keys;
            val[e] = 0u;
            pw[e] = has ? 0xFFFFFFFFu : 0u;
            if (has) val[e] = as_global(a.values)[row];
            if (has && a.present) pw[e] = as_global(a.present)[row >> 5];
        }
        uint32_t slot[4];
        unsigned long long w[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            slot[e] = kAggNoSlot;
            w[e] = 0ull;
            if ((v << 2) + e >= local_len) continue;  // the padding, or behind the set
            if (agg_bit(pw[e], id[e] - a.key_base)) slot[e] = agg_value(val[e], a.n_edges, s, l, &w[e]);
            else ++l.other;  // a doc of the set without a value
        }
        agg_sum<kPre>(s, slot, w);
    }
    agg_flush(s, a, l, state, mm);
}

// aggs[f]: a column keyed by value id (16-byte aligned values with a vector of slack behind them) with its value_id_to_anchor table and its zeroed
// has_bits.  member: words with doc d's bit in word (d >> 5) - member_word0, valid for every d in [doc_lo, doc_hi)
template <bool kPre>
__global__ __launch_bounds__(64) void k_docset_agg_values(const DocsetAggD* __restrict__ aggs, const uint32_t* __restrict__ member, uint32_t member_word0, uint32_t doc_lo,
                                                          uint32_t doc_hi, unsigned long long* __restrict__ state, uint32_t* __restrict__ mm) {
    VQ_AGG_LDS;
    const uint32_t lane = lane_id();
    const DocsetAggD a = aggs[blockIdx.y];  // (uniform)
    agg_init(s, a);
    AggLane l;
    const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(a.values));
    const unsigned long long nvec = ((unsigned long long)a.num_keys + 3u) >> 2;
    for (unsigned long long v0 = (unsigned long long)blockIdx.x * 64u; v0 < nvec; v0 += (unsigned long long)gridDim.x * 64u) {  // (uniform trip count)
        const unsigned long long v = v0 + lane;
        const bool in = v < nvec;
        u32x4 d = u32x4{0u, 0u, 0u, 0u};
        if (in) d = vec[v];
        const uint32_t r0 = (uint32_t)(v << 2);  // (a multiple of 4: its four rows share a presence word)
        uint32_t pw = in ? 0xFFFFFFFFu : 0u;
        if (in && a.present) pw = as_global(a.present)[r0 >> 5];
        const uint32_t val[4] = {d.x, d.y, d.z, d.w};
        uint32_t anchor[4], mark = 0;  // bit e: a present value with a row in the table / with an anchor / of a doc of the set
        unsigned long long first[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const uint32_t r = r0 + e;
            const unsigned long long vid = (unsigned long long)a.key_base + r, arow = vid - a.a_key_base;
            first[e] = 0ull;
            if (in && r < a.num_keys && agg_bit(pw, r) && vid >= a.a_key_base && arow < a.a_num_keys) {
                first[e] = as_global(a.a_off)[arow];
                if (first[e] < as_global(a.a_off)[arow + 1u]) mark |= 1u << e;  // (an empty row belongs to nobody)
            }
        }
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            anchor[e] = 0xFFFFFFFFu;
            if ((mark >> e) & 1u) anchor[e] = as_global(a.a_vals)[first[e]];
        }
        uint32_t mw[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            mw[e] = 0u;
            if (anchor[e] >= doc_lo && anchor[e] < doc_hi) mw[e] = as_global(member)[(anchor[e] >> 5) - member_word0];
        }
        uint32_t slot[4];
        unsigned long long w[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            slot[e] = kAggNoSlot;
            w[e] = 0ull;
            if (!agg_bit(mw[e], anchor[e])) continue;  // (outside the doc range: mw is 0)
            const uint32_t bit = 1u << (anchor[e] & 31u);
            if (!(atomicOr(a.has_bits + (anchor[e] >> 5), bit) & bit)) ++l.other;  // the doc's first present value
            slot[e] = agg_value(val[e], a.n_edges, s, l, &w[e]);
        }
        agg_sum<kPre>(s, slot, w);
    }
    agg_flush(s, a, l, state, mm);
}

void launch_docset_agg_ids(hipStream_t st, const uint32_t* docs, uint32_t local_len, const DocsetAggD* aggs, uint32_t m, unsigned long long* state, uint32_t* mm, bool prereduce,
                           uint32_t max_grid) {
    if (!local_len || !m || m > 65535u) return;
    const uint64_t waves = ((uint64_t(local_len) + 3u) / 4u + 63u) / 64u;
    const dim3 grid(uint32_t(std::min<uint64_t>(waves, max_grid ? std::min(max_grid, kAggMaxGrid) : kAggMaxGrid)), m);
    if (prereduce) hipLaunchKernelGGL(k_docset_agg_ids<true>, grid, dim3(64), 0, st, docs, local_len, aggs, state, mm);
    else hipLaunchKernelGGL(k_docset_agg_ids<false>, grid, dim3(64), 0, st, docs, local_len, aggs, state, mm);
}
void launch_docset_agg_values(hipStream_t st, const DocsetAggD* aggs, uint32_t m, uint32_t max_keys, const uint32_t* member, uint32_t member_word0, uint32_t doc_lo,
                              uint32_t doc_hi, unsigned long long* state, uint32_t* mm, bool prereduce, uint32_t max_grid) {
    if (!m || m > 65535u || !max_keys || !member || doc_hi <= doc_lo) return;
    const uint64_t waves = ((uint64_t(max_keys) + 3u) / 4u + 63u) / 64u;
    const dim3 grid(uint32_t(std::min<uint64_t>(waves, max_grid ? std::min(max_grid, kAggMaxGrid) : kAggMaxGrid)), m);
    if (prereduce) hipLaunchKernelGGL(k_docset_agg_values<true>, grid, dim3(64), 0, st, aggs, member, member_word0, doc_lo, doc_hi, state, mm);
    else hipLaunchKernelGGL(k_docset_agg_values<false>, grid, dim3(64), 0, st, aggs, member, member_word0, doc_lo, doc_hi, state, mm);
}

}  // namespace vq
