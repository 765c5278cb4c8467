// Doc sets ordered by a column: the first K rows of a staged set's docs in the order (sort key ascending, doc ascending), selected on the device
// (DocsetTopD, the sort key and the state layout: kernels.hpp).  Plain kernels on one stream; one wave64 per workgroup, grids capped and strided;
// no workgroup waits for another; 16 B per lane on every stream; integer compares and integer atomics only — no float is compared anywhere, and
// nothing the host reads depends on the order of the atomics: the histograms and counters are sums, the fold is a minimum, the cursor hands out
// slots of a part of the output whose order the final sort decides.
//
//   k_top_fold      1:n columns: lanes stream the value column 16 B at a time like k_docset_agg_values; a present value whose anchor is a member
//                   of the set does atomicMin of its sort key on best[anchor - doc_lo] (preset to the missing key).
//   k_top_keys      lanes stream DocSet::docs four ids at a time (bounded by local_len), gather value and presence (or the folded key), write the
//                   sort keys coalesced, count the top byte in a 256-bin LDS histogram (hist_add) and count / nan / missing in registers; non-zero
//                   state goes to HBM once per workgroup.
//   k_top_pick      one wave: four bins per lane, a wave scan finds the bin where the running count reaches the rows still wanted; the agreed
//                   prefix grows by that digit and the want shrinks by the keys below it.  After the last digit: T, B, E, take, all-ties.
//   k_top_hist      streams the keys (not the column) and counts the next byte of those that match the prefix.
//   k_top_tiecount  workgroup c counts the keys == T of its contiguous chunk; leaves at once when E == take (or nothing is wanted).
//   k_top_emit      workgroup c walks the same chunk: keys < T take slots from one returning atomic cursor (one atomic per wave and round, only
//                   when the round holds any); keys == T are ranked by the chunks in front (summed by the wave itself), a wave scan and the
//                   lane's own order, and the first `take` go to out[B + rank]: ascending doc id, because docs is sorted and chunks are contiguous.
#include <algorithm>

#include "kernel_common.hpp"
#include "kernels.hpp"

namespace vq {

__device__ __forceinline__ bool top_bit(uint32_t word, uint32_t at) { return (word >> (at & 31u)) & 1u; }
__device__ __forceinline__ uint32_t top_key(uint32_t bits, uint32_t descending) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return kTopNanKey;
    const uint32_t k = range_key(bits);
    return descending ? ~k : k;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(x), 63); }

// a: a column keyed by value id with its value_id_to_anchor table.  member: words with doc d's bit in word (d >> 5) - member_word0, valid for every
// d in [a.doc_lo, doc_hi).  best: doc_hi - a.doc_lo words
__global__ __launch_bounds__(64) void k_top_fold(DocsetTopD a, const uint32_t* __restrict__ member, uint32_t member_word0, uint32_t doc_hi, uint32_t* __restrict__ best) {
    const uint32_t lane = lane_id();
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
        uint32_t anchor[4], mark = 0;  // bit e: a present value with an anchor
        unsigned long long first[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const uint32_t r = r0 + e;
            const unsigned long long vid = (unsigned long long)a.key_base + r, arow = vid - a.a_key_base;
            first[e] = 0ull;
            if (in && r < a.num_keys && top_bit(pw, r) && vid >= a.a_key_base && arow < a.a_num_keys) {
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
            if (anchor[e] >= a.doc_lo && anchor[e] < doc_hi) mw[e] = as_global(member)[(anchor[e] >> 5) - member_word0];
        }
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e)
            if (top_bit(mw[e], anchor[e])) atomicMin(best + (anchor[e] - a.doc_lo), top_key(val[e], a.descending));  // (outside the doc range: mw is 0)
    }
}

// docs: 16-byte aligned, (local_len + 3) / 4 whole vectors, every real entry inside the index's doc range; keys: as many vectors; hist, state zeroed
__global__ __launch_bounds__(64) void k_top_keys(const uint32_t* __restrict__ docs, uint32_t local_len, DocsetTopD a, uint32_t* __restrict__ keys, uint32_t* __restrict__ hist,
                                                 uint32_t* __restrict__ state) {
    __shared__ uint32_t lds_hist[256];
    const uint32_t lane = lane_id();
    for (uint32_t i = lane; i < 256u; i += 64u) lds_hist[i] = 0u;
    __syncthreads();
    uint32_t c_num = 0, c_nan = 0, c_miss = 0;
    const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(docs));
    u32x4* kvec = reinterpret_cast<u32x4*>(keys);
    const unsigned long long nvec = ((unsigned long long)local_len + 3u) >> 2;
    for (unsigned long long v0 = (unsigned long long)blockIdx.x * 64u; v0 < nvec; v0 += (unsigned long long)gridDim.x * 64u) {  // (uniform trip count)
        const unsigned long long v = v0 + lane;
        u32x4 d = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (v < nvec) d = vec[v];
        const uint32_t id[4] = {d.x, d.y, d.z, d.w};
        uint32_t key[4];
        if (a.best) {  // (uniform)
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e) {
                key[e] = kTopMissingKey;
                if ((v << 2) + e < local_len) key[e] = as_global(a.best)[id[e] - a.doc_lo];
            }
        } else {
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
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e) key[e] = top_bit(pw[e], id[e] - a.key_base) ? top_key(val[e], a.descending) : kTopMissingKey;
        }
        if (v < nvec) kvec[v] = u32x4{key[0], key[1], key[2], key[3]};  // (the padding of the last vector holds the missing key)
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const bool in = (v << 2) + e < local_len;  // the padding, or behind the set: never counted
            c_num += in && key[e] <= kRangeKeyMax;
            c_nan += in && key[e] == kTopNanKey;
            c_miss += in && key[e] == kTopMissingKey;
            hist_add(lds_hist, in, key[e] >> 24);
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < 256u; i += 64u)
        if (lds_hist[i]) atomicAdd(hist + i, lds_hist[i]);
    c_num = wave_sum_u32(c_num);
    c_nan = wave_sum_u32(c_nan);
    c_miss = wave_sum_u32(c_miss);
    if (lane == 0u) {
        if (c_num) atomicAdd(state + kTopCount, c_num);
        if (c_nan) atomicAdd(state + kTopNan, c_nan);
        if (c_miss) atomicAdd(state + kTopMissing, c_miss);
    }
}

__global__ __launch_bounds__(64) void k_top_pick(uint32_t* __restrict__ state, const uint32_t* __restrict__ hist, uint32_t shift, uint32_t rows, uint32_t with_missing,
                                                 uint32_t n) {
    const uint32_t lane = lane_id();
    if (state[kTopDone]) return;  // (uniform)
    uint32_t want = state[kTopWant], prefix = state[kTopPrefix], below = state[kTopB];
    if (shift == 24u) {
        const uint32_t eligible = with_missing ? n : state[kTopCount];
        want = rows < eligible ? rows : eligible;
        prefix = 0u;
        below = 0u;
    }
    const uint32_t h0 = hist[4u * lane], h1 = hist[4u * lane + 1u], h2 = hist[4u * lane + 2u], h3 = hist[4u * lane + 3u];
    const uint32_t mine = h0 + h1 + h2 + h3;
    uint32_t total;
    const uint32_t before = wave_excl_scan_u32(mine, &total);
    const unsigned long long reach = __ballot(before + mine >= want);
    if (want == 0u || !reach) {  // nothing is wanted (a histogram that does not reach the want cannot occur: the want never exceeds its total)
        if (lane == 0u) {
            state[kTopT] = 0u;
            state[kTopB] = 0u;
            state[kTopE] = 0u;
            state[kTopTake] = 0u;
            state[kTopAllTies] = 0u;
            state[kTopWant] = 0u;
            state[kTopDone] = 1u;
        }
        return;
    }
    if (lane != (uint32_t)__builtin_ctzll(reach)) return;
    uint32_t seen = before, bin = 4u * lane, here = h0;
    if (seen + here < want) {
        seen += here;
        ++bin;
        here = h1;
        if (seen + here < want) {
            seen += here;
            ++bin;
            here = h2;
            if (seen + here < want) {
                seen += here;
                ++bin;
                here = h3;
            }
        }
    }
    prefix |= bin << shift;
    state[kTopPrefix] = prefix;
    state[kTopWant] = want - seen;
    state[kTopB] = below + seen;
    if (shift == 0u) {
        state[kTopT] = prefix;
        state[kTopE] = here;
        state[kTopTake] = want - seen;
        state[kTopAllTies] = here == want - seen ? 1u : 0u;
    }
}

// keys: (n + 3) / 4 whole vectors
__global__ __launch_bounds__(64) void k_top_hist(const uint32_t* __restrict__ keys, uint32_t n, uint32_t shift, const uint32_t* __restrict__ state,
                                                 uint32_t* __restrict__ hist) {
    __shared__ uint32_t lds_hist[256];
    if (state[kTopDone]) return;  // (uniform)
    const uint32_t lane = lane_id();
    for (uint32_t i = lane; i < 256u; i += 64u) lds_hist[i] = 0u;
    __syncthreads();
    const uint32_t prefix = state[kTopPrefix], mask = 0xFFFFFFFFu << (shift + 8u);  // (shift <= 16)
    const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(keys));
    const unsigned long long nvec = ((unsigned long long)n + 3u) >> 2;
    for (unsigned long long v0 = (unsigned long long)blockIdx.x * 64u; v0 < nvec; v0 += (unsigned long long)gridDim.x * 64u) {  // (uniform trip count)
        const unsigned long long v = v0 + lane;
        u32x4 d = u32x4{0u, 0u, 0u, 0u};
        if (v < nvec) d = vec[v];
        const uint32_t key[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) hist_add(lds_hist, (v << 2) + e < n && (key[e] & mask) == prefix, (key[e] >> shift) & 0xFFu);
    }
    __syncthreads();
    for (uint32_t i = lane; i < 256u; i += 64u)
        if (lds_hist[i]) atomicAdd(hist + i, lds_hist[i]);
}

__global__ __launch_bounds__(64) void k_top_tiecount(const uint32_t* __restrict__ keys, uint32_t n, unsigned long long vpc, const uint32_t* __restrict__ state,
                                                     uint32_t* __restrict__ chunks) {
    if (state[kTopDone] || state[kTopAllTies] || !state[kTopTake]) return;  // (uniform) all ties are taken, or none: nobody reads the chunk counts
    const uint32_t lane = lane_id(), T = state[kTopT];
    const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(keys));
    const unsigned long long nvec = ((unsigned long long)n + 3u) >> 2;
    const unsigned long long lo = (unsigned long long)blockIdx.x * vpc, end = lo + vpc, hi = end < nvec ? end : nvec;
    uint32_t mine = 0;
    for (unsigned long long v0 = lo; v0 < hi; v0 += 64u) {  // (uniform trip count)
        const unsigned long long v = v0 + lane;
        if (v >= hi) continue;
        const u32x4 d = vec[v];
        const uint32_t key[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) mine += (v << 2) + e < n && key[e] == T;
    }
    mine = wave_sum_u32(mine);
    if (lane == 0u) chunks[blockIdx.x] = mine;
}

__global__ __launch_bounds__(64) void k_top_emit(const uint32_t* __restrict__ docs, const uint32_t* __restrict__ keys, uint32_t n, unsigned long long vpc,
                                                 uint32_t* __restrict__ state, const uint32_t* __restrict__ chunks, unsigned long long* __restrict__ out, uint32_t cap) {
    if (state[kTopDone]) return;  // (uniform)
    const uint32_t lane = lane_id(), T = state[kTopT], B = state[kTopB], all = state[kTopAllTies], take = all ? 0u : state[kTopTake];
    uint32_t eq_before = 0;
    if (take) {  // (uniform) the ties of the chunks in front of this one
        uint32_t mine = 0;
        for (uint32_t c = lane; c < blockIdx.x; c += 64u) mine += chunks[c];
        eq_before = wave_sum_u32(mine);
    }
    const VQ_GLOBAL u32x4* kvec = as_global(reinterpret_cast<const u32x4*>(keys));
    const VQ_GLOBAL u32x4* dvec = as_global(reinterpret_cast<const u32x4*>(docs));
    const unsigned long long nvec = ((unsigned long long)n + 3u) >> 2;
    const unsigned long long lo = (unsigned long long)blockIdx.x * vpc, end = lo + vpc, hi = end < nvec ? end : nvec;
    for (unsigned long long v0 = lo; v0 < hi; v0 += 64u) {  // (uniform trip count)
        const unsigned long long v = v0 + lane;
        u32x4 k = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, d = k;
        if (v < hi) {
            k = kvec[v];
            d = dvec[v];
        }
        const uint32_t key[4] = {k.x, k.y, k.z, k.w}, doc[4] = {d.x, d.y, d.z, d.w};
        uint32_t low = 0, eq = 0;  // bit e: entry e goes through the cursor / is a tie that is ranked
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) {
            const bool in = v < hi && (v << 2) + e < n;
            if (in && (key[e] < T || (all && key[e] == T))) low |= 1u << e;
            if (in && !all && key[e] == T) eq |= 1u << e;
        }
        uint32_t total;
        uint32_t at = wave_excl_scan_u32((uint32_t)__popc(low), &total);
        if (total) {  // (uniform)
            uint32_t base = 0;
            if (lane == 0u) base = atomicAdd(state + kTopCursor, total);
            at += (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e)
                if ((low >> e) & 1u) {
                    if (at < cap) out[at] = ((unsigned long long)key[e] << 32) | doc[e];
                    ++at;
                }
        }
        if (eq_before < take) {  // (uniform)
            uint32_t ties;
            uint32_t rank = eq_before + wave_excl_scan_u32((uint32_t)__popc(eq), &ties);
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e)
                if ((eq >> e) & 1u) {
                    if (rank < take && B + rank < cap) out[B + rank] = ((unsigned long long)key[e] << 32) | doc[e];
                    ++rank;
                }
            eq_before += ties;
        }
    }
}

void launch_top_fold(hipStream_t st, const DocsetTopD& a, const uint32_t* member, uint32_t member_word0, uint32_t doc_hi, uint32_t* best, uint32_t max_grid) {
    if (!a.num_keys || !member || !best || doc_hi <= a.doc_lo) return;
    const uint32_t grid = top_grid((uint64_t(a.num_keys) + 3u) / 4u, max_grid);
    hipLaunchKernelGGL(k_top_fold, dim3(grid), dim3(64), 0, st, a, member, member_word0, doc_hi, best);
}
void launch_top_keys(hipStream_t st, const uint32_t* docs, uint32_t local_len, const DocsetTopD& a, uint32_t* keys, uint32_t* hist, uint32_t* state, uint32_t max_grid) {
    if (!local_len) return;
    const uint32_t grid = top_grid((uint64_t(local_len) + 3u) / 4u, max_grid);
    hipLaunchKernelGGL(k_top_keys, dim3(grid), dim3(64), 0, st, docs, local_len, a, keys, hist, state);
}
void launch_top_pick(hipStream_t st, uint32_t* state, const uint32_t* hist, uint32_t shift, uint32_t rows, bool with_missing, uint32_t n) {
    hipLaunchKernelGGL(k_top_pick, dim3(1), dim3(64), 0, st, state, hist, shift, rows, with_missing ? 1u : 0u, n);
}
void launch_top_hist(hipStream_t st, const uint32_t* keys, uint32_t n, uint32_t shift, const uint32_t* state, uint32_t* hist, uint32_t max_grid) {
    if (!n || shift > 16u) return;
    const uint32_t grid = top_grid((uint64_t(n) + 3u) / 4u, max_grid);
    hipLaunchKernelGGL(k_top_hist, dim3(grid), dim3(64), 0, st, keys, n, shift, state, hist);
}
void launch_top_tiecount(hipStream_t st, const uint32_t* keys, uint32_t n, const uint32_t* state, uint32_t* chunks, uint32_t max_grid) {
    if (!n) return;
    const uint64_t nvec = (uint64_t(n) + 3u) / 4u;
    const uint32_t grid = top_grid(nvec, max_grid);
    hipLaunchKernelGGL(k_top_tiecount, dim3(grid), dim3(64), 0, st, keys, n, (unsigned long long)((nvec + grid - 1u) / grid), state, chunks);
}
void launch_top_emit(hipStream_t st, const uint32_t* docs, const uint32_t* keys, uint32_t n, uint32_t* state, const uint32_t* chunks, unsigned long long* out, uint32_t cap,
                     uint32_t max_grid) {
    if (!n || !cap) return;
    const uint64_t nvec = (uint64_t(n) + 3u) / 4u;
    const uint32_t grid = top_grid(nvec, max_grid);
    hipLaunchKernelGGL(k_top_emit, dim3(grid), dim3(64), 0, st, docs, keys, n, (unsigned long long)((nvec + grid - 1u) / grid), state, chunks, out, cap);
}

}  // namespace vq
