// Facet counts of a doc set: the histogram of every requested facet over a staged set's local ids (DocSet::docs: sorted, unique, padded to a
// multiple of 4 entries with 0xFFFFFFFF).  The semantics are those of the scans' facet sink stage (kernels.hip, persistence.rs:164-175
// count_values_for_ids): row = id - key_base, rows >= num_keys add nothing; a direct store adds its value unless that is 0xFFFFFFFF; a CSR row
// adds one per entry, duplicates included; a value >= num_values is skipped.  Counters are u32 and every sum is an integer: the result does not
// depend on the order of the atomics.
//
//   k_docset_facet_count   grid (x, m): workgroup (x, f) counts facet f over its stride of the ids.  One wave64 per workgroup, the grid capped and
//                          strided; no workgroup waits for another; plain loads, vector stores and atomics only.  Lanes stream the ids 16 B at a
//                          time (four ids per lane and round, bounded by local_len: the padding is never counted), fetch the four rows' offsets
//                          (or direct values) together, then count.  A CSR row of more than kDocsetFacetLaneRow entries is not walked by its lane:
//                          the wave takes such rows one after the other, 64 entries per round.
//                          Two counting modes, chosen per facet by the host (DocsetFacetD::lds):
//                            LDS mode     num_values <= kDocsetFacetLdsValues: the whole histogram lives in LDS, counting is LDS atomics only, the
//                                         non-zero counters are added to HBM once, at the end of the workgroup's stride.
//                            cache mode   longer histograms: a direct-mapped counter cache of kDocsetFacetCache slots (slot by hash, CAS on the key,
//                                         a miss adds straight to HBM), flushed once at the end — the scans' facet_add / facet_cache_flush restated.
//   launch_docset_facet_rank   the selection that follows: the search's own k_facet_select / k_facet_select_wide over the summed histograms.
#include <algorithm>

#include "kernel_common.hpp"
#include "kernels.hpp"

namespace vq {

constexpr uint32_t kDocsetFacetMaxGrid = 2048;  // workgroups of one wave per facet: what the chip holds at once (LDS: 10 per CU); the rest is strided
constexpr uint32_t kDocsetFacetLaneRow = 32;    // entries of a CSR row one lane walks alone
constexpr uint32_t kDocsetFacetCache = 1024;    // slots of the cache mode's counter cache (keys + counts: 8 KB of the same LDS)
static_assert(2u * kDocsetFacetCache <= kDocsetFacetLdsValues, "the counter cache lives in the LDS histogram's space");

struct DocsetFacetCounter {
    uint32_t* lds;   // LDS mode: the histogram; cache mode: keys [0, kDocsetFacetCache), counts behind them
    uint32_t* hist;  // the facet's histogram in HBM
    uint32_t num_values;
    bool in_lds;  // (uniform)
    __device__ __forceinline__ void add(uint32_t v) const {
        if (v >= num_values) return;
        if (in_lds) {
            atomicAdd(&lds[v], 1u);
            return;
        }
        const uint32_t slot = (v * 2654435761u) >> 22;
        const uint32_t old = atomicCAS(&lds[slot], 0xFFFFFFFFu, v);
        if (old == 0xFFFFFFFFu || old == v) atomicAdd(&lds[kDocsetFacetCache + slot], 1u);
        else atomicAdd(&hist[v], 1u);
    }
};

// docs: 16-byte aligned, (local_len + 3) / 4 whole vectors; hist: zeroed before the launch, facet f's counters from facets[f].hist_off on
__global__ __launch_bounds__(64) void k_docset_facet_count(const uint32_t* __restrict__ docs, uint32_t local_len, const DocsetFacetD* __restrict__ facets,
                                                           uint32_t* __restrict__ hist) {
    __shared__ uint32_t lds[kDocsetFacetLdsValues];
    const uint32_t lane = lane_id();
    const DocsetFacetD fa = facets[blockIdx.y];  // (uniform)
    const DocsetFacetCounter cnt{lds, hist + fa.hist_off, fa.num_values, fa.lds != 0u};
    if (cnt.in_lds) {
        for (uint32_t v = lane; v < fa.num_values; v += 64u) lds[v] = 0u;
    } else {
        for (uint32_t s = lane; s < kDocsetFacetCache; s += 64u) {
            lds[s] = 0xFFFFFFFFu;
            lds[kDocsetFacetCache + s] = 0u;
        }
    }
    __syncthreads();
    const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(docs));
    const unsigned long long nvec = ((unsigned long long)local_len + 3u) >> 2;
    for (unsigned long long v0 = (unsigned long long)blockIdx.x * 64u; v0 < nvec; v0 += (unsigned long long)gridDim.x * 64u) {  // (uniform trip count)
        const unsigned long long v = v0 + lane;
        u32x4 d = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (v < nvec) d = vec[v];
        const uint32_t id[4] = {d.x, d.y, d.z, d.w};
        uint32_t row[4];
        bool live[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            row[k] = id[k] - fa.key_base;  // (unsigned: an id below key_base becomes a row >= num_keys)
            live[k] = (v << 2) + k < local_len && row[k] < fa.num_keys;
        }
        if (fa.direct) {  // (uniform) a scalar field: one gather per id
            uint32_t val[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) val[k] = live[k] ? as_global(fa.direct)[row[k]] : 0xFFFFFFFFu;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) cnt.add(val[k]);  // (0xFFFFFFFF >= num_values: no value)
            continue;
        }
        unsigned long long e0[4], e1[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            e0[k] = live[k] ? as_global(fa.offsets)[row[k]] : 0ull;
            e1[k] = live[k] ? as_global(fa.offsets)[row[k] + 1u] : 0ull;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const bool is_long = e1[k] - e0[k] > (unsigned long long)kDocsetFacetLaneRow;
            if (!is_long)
                for (unsigned long long e = e0[k]; e < e1[k]; ++e) cnt.add(as_global(fa.values)[e]);
            unsigned long long pending = __ballot(is_long);  // (uniform) the long rows: the wave walks each, 64 entries per round
            while (pending) {
                const uint32_t src = (uint32_t)__ffsll((long long)pending) - 1u;
                pending &= pending - 1ull;
                const unsigned long long b = shfl_u64(e0[k], src), e = shfl_u64(e1[k], src);
                for (unsigned long long at = b + lane; at < e; at += 64u) cnt.add(as_global(fa.values)[at]);
            }
        }
    }
    __syncthreads();
    if (cnt.in_lds) {
        for (uint32_t v = lane; v < fa.num_values; v += 64u) {
            const uint32_t c = lds[v];
            if (c) atomicAdd(&cnt.hist[v], c);
        }
    } else {
        for (uint32_t s = lane; s < kDocsetFacetCache; s += 64u) {
            const uint32_t key = lds[s];
            if (key != 0xFFFFFFFFu) atomicAdd(&cnt.hist[key], lds[kDocsetFacetCache + s]);
        }
    }
}

void launch_docset_facet_count(hipStream_t st, const uint32_t* docs, uint32_t local_len, const DocsetFacetD* facets, uint32_t m, uint32_t* hist) {
    if (!local_len || !m) return;
    const uint64_t waves = ((uint64_t(local_len) + 3u) / 4u + 63u) / 64u;
    hipLaunchKernelGGL(k_docset_facet_count, dim3(uint32_t(std::min<uint64_t>(waves, kDocsetFacetMaxGrid)), m), dim3(64), 0, st, docs, local_len, facets, hist);
}
void launch_docset_facet_rank(hipStream_t st, uint32_t n_jobs, const FacetJob* jobs, const uint32_t* hist, uint32_t* out_vals, uint32_t* out_counts, uint32_t* out_n) {
    launch_facet_select(st, n_jobs, jobs, hist, out_vals, out_counts, out_n);
}

}  // namespace vq
