// Dense union (K2, wide leaves): the union of a leaf's posting lists with the per-doc maximum of term_score * (f16 / 100), for leaves
// that match more lists than two levels of k_union take (kernels.hip).  Cost: O(postings + docs of the shard's range), whatever the
// number of lists.
//
//   scatter  one u32 key per doc of the shard's range [lo, lo + range) lives in the job's slab (zeroed before).  The lists of a group of
//            jobs are flattened by a prefix sum of their lengths (UDenseList::first); a workgroup takes 1024 consecutive postings,
//            whichever lists they belong to.  key = order_f32(value), raised with a no-return atomic max: a maximum does not depend
//            on the order of arrival, so the result is bit-exact and reproducible.
//   count    present docs (key != 0) and the largest key per block of 2048 slab words.
//   offsets  exclusive prefix sums of a job's block counts, in place; the job's length and its largest key (== its largest value).
//   write    (doc, value) in ascending doc order in k_union<write>'s format: 8 sentinel entries (0xFFFFFFFF, 0.0f) behind the list.
//
// The empty slab word is 0.  order_f32 maps exactly one bit pattern there, the NaN 0xFFFFFFFF; no arithmetic on f16 scores and term
// scores yields it (hardware NaNs are 0x7FC00000 / 0xFFC00000 or an operand's payload), and it is stored as key 1 (the NaN 0xFFFFFFFE).
// 0.0, -0.0 and the negative values of a negative leaf boost all have keys of their own above 0.
#include "kernel_common.hpp"
#include "kernels.hpp"

namespace vq {

constexpr uint32_t kDenseThreads = 256;
constexpr uint32_t kDenseTile = 1024;                                 // postings per scatter workgroup
constexpr uint32_t kDensePerThread = kDenseBlockDocs / kDenseThreads;  // slab words per thread of count / write
static_assert(kDensePerThread == 8, "count / write read two 16-byte vectors per thread");

// The first list of [0, n) whose postings reach beyond flattened posting p (lists[n].first == total > p).
__device__ __forceinline__ uint32_t dense_list_of(const VQ_GLOBAL UDenseList* lists, uint32_t n, unsigned long long p) {
    uint32_t lo = 0, hi = n;  // invariant: lists[lo].first <= p < lists[hi].first
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lists[mid].first <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kDenseThreads) void k_union_dense_scatter(const UDenseList* __restrict__ lists_, uint32_t n_lists, const UDenseJob* __restrict__ jobs_,
                                                                        uint32_t* __restrict__ slab, uint32_t lo_doc, uint32_t range) {
    __shared__ uint32_t rel[kDenseTile + 1];  // first posting of list l0 + k, relative to the tile (clamped to [0, kDenseTile])
    const VQ_GLOBAL UDenseList* lists = as_global(lists_);
    const VQ_GLOBAL UDenseJob* jobs = as_global(jobs_);
    const unsigned long long total = lists[n_lists].first;
    const unsigned long long tile = (unsigned long long)blockIdx.x * kDenseTile;
    if (tile >= total) return;
    const uint32_t l0 = dense_list_of(lists, n_lists, tile);  // (uniform)
    // every list is non-empty: the tile's postings belong to at most kDenseTile lists
    const uint32_t nl = min(n_lists - l0, kDenseTile);
    for (uint32_t k = threadIdx.x; k <= nl; k += kDenseThreads) {
        const unsigned long long f = lists[l0 + k].first;
        rel[k] = f <= tile ? 0u : (uint32_t)min(f - tile, (unsigned long long)kDenseTile);
    }
    __syncthreads();
    const uint32_t in_tile = (uint32_t)min(total - tile, (unsigned long long)kDenseTile);
    for (uint32_t q = threadIdx.x; q < in_tile; q += kDenseThreads) {
        uint32_t a = 0, b = nl;  // rel[a] <= q < rel[b]  (rel[nl] is the next list's first posting, or the tile's end)
        while (b - a > 1u) {
            const uint32_t mid = (a + b) >> 1;
            if (rel[mid] <= q) a = mid;
            else b = mid;
        }
        const VQ_GLOBAL UDenseList* L = lists + l0 + a;
        const unsigned long long i = tile + q - L->first;
        const uint32_t doc = as_global(L->docs)[i];
        const float v = posting_value(L->term_score, as_global(L->scores)[i]);
        const uint32_t d = doc - lo_doc;
        if (d < range) {
            uint32_t key = order_f32(__float_as_uint(v));
            key = key ? key : 1u;
            (void)__hip_atomic_fetch_max(slab + jobs[L->job].slab_off + d, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// the job of compact block b (uniform): jobs[j].block_begin <= b < jobs[j + 1].block_begin
__device__ __forceinline__ uint32_t dense_job_of(const VQ_GLOBAL UDenseJob* jobs, uint32_t n_jobs, uint32_t b) {
    uint32_t jl = 0, jh = n_jobs;
    while (jh - jl > 1u) {
        const uint32_t mid = (jl + jh) >> 1;
        if (jobs[mid].block_begin <= b) jl = mid;
        else jh = mid;
    }
    return jl;
}

__device__ __forceinline__ uint32_t block_sum_u32(uint32_t x, uint32_t* sh /* [kDenseThreads / 64] */) {
    for (uint32_t off = 32; off > 0; off >>= 1) x += (uint32_t)__shfl_xor((int)x, (int)off);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}
static_assert(kDenseThreads == 256, "block_sum_u32 adds four waves");

__global__ __launch_bounds__(kDenseThreads) void k_union_dense_count(const UDenseJob* __restrict__ jobs_, uint32_t n_jobs, const uint32_t* __restrict__ slab,
                                                                      uint32_t* __restrict__ block_cnt, uint32_t* __restrict__ block_max) {
    __shared__ uint32_t sh[kDenseThreads / 64], shm[kDenseThreads / 64];
    const VQ_GLOBAL UDenseJob* jobs = as_global(jobs_);
    const uint32_t j = dense_job_of(jobs, n_jobs, blockIdx.x);
    const UDenseJob J = jobs_[j];
    const VQ_GLOBAL u32x4* w = (const VQ_GLOBAL u32x4*)(slab + J.slab_off + (unsigned long long)(blockIdx.x - J.block_begin) * kDenseBlockDocs) + threadIdx.x * 2u;
    const u32x4 x = w[0], y = w[1];  // (the slab is padded to whole blocks)
    const uint32_t c = (x.x != 0) + (x.y != 0) + (x.z != 0) + (x.w != 0) + (y.x != 0) + (y.y != 0) + (y.z != 0) + (y.w != 0);
    uint32_t m = max(max(max(x.x, x.y), max(x.z, x.w)), max(max(y.x, y.y), max(y.z, y.w)));
    for (uint32_t off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, (int)off));
    if ((threadIdx.x & 63u) == 0) shm[threadIdx.x >> 6] = m;
    const uint32_t n = block_sum_u32(c, sh);
    if (threadIdx.x == 0) {  // (a word per block, not one atomic max per block on the job's word: thousands of blocks on one address serialise)
        block_cnt[blockIdx.x] = n;
        block_max[blockIdx.x] = max(max(shm[0], shm[1]), max(shm[2], shm[3]));
    }
}

// one workgroup per job: block counts -> exclusive offsets (in place), the total -> the job's length; the blocks' largest keys -> the job's
__global__ __launch_bounds__(kDenseThreads) void k_union_dense_offsets(const UDenseJob* __restrict__ jobs_, uint32_t* __restrict__ block_cnt, const uint32_t* __restrict__ block_max,
                                                                        UDenseResult* __restrict__ results) {
    __shared__ uint32_t sh[kDenseThreads / 64], shm[kDenseThreads / 64];
    const UDenseJob J = jobs_[blockIdx.x];
    uint32_t* cnt = block_cnt + J.block_begin;
    uint32_t carry = 0, m = 0;
    for (uint32_t base = 0; base < J.n_blocks; base += kDenseThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < J.n_blocks ? cnt[i] : 0u;
        if (i < J.n_blocks) m = max(m, block_max[J.block_begin + i]);
        uint32_t wave_total;
        const uint32_t ex = wave_excl_scan_u32(c, &wave_total);
        __syncthreads();  // (the previous round's sh has been read)
        if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = wave_total;
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t wv = 0; wv < (threadIdx.x >> 6); ++wv) before += sh[wv];
        if (i < J.n_blocks) cnt[i] = carry + before + ex;
        carry += sh[0] + sh[1] + sh[2] + sh[3];
    }
    for (uint32_t off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, (int)off));
    if ((threadIdx.x & 63u) == 0) shm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        results[J.result].len = carry;
        results[J.result].max_key = max(max(shm[0], shm[1]), max(shm[2], shm[3]));
    }
}

__global__ __launch_bounds__(kDenseThreads) void k_union_dense_write(const UDenseJob* __restrict__ jobs_, uint32_t n_jobs, const uint32_t* __restrict__ slab,
                                                                      const uint32_t* __restrict__ block_off, uint32_t lo_doc, uint32_t* __restrict__ out_docs,
                                                                      float* __restrict__ out_vals) {
    __shared__ uint32_t sh[kDenseThreads / 64];
    const VQ_GLOBAL UDenseJob* jobs = as_global(jobs_);
    const uint32_t j = dense_job_of(jobs, n_jobs, blockIdx.x);
    const UDenseJob J = jobs_[j];
    const uint32_t b = blockIdx.x - J.block_begin;
    const VQ_GLOBAL u32x4* w = (const VQ_GLOBAL u32x4*)(slab + J.slab_off + (unsigned long long)b * kDenseBlockDocs) + threadIdx.x * 2u;
    const u32x4 x = w[0], y = w[1];
    const uint32_t k[kDensePerThread] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    uint32_t c = 0;
#pragma unroll
    for (uint32_t i = 0; i < kDensePerThread; ++i) c += k[i] != 0;
    uint32_t wave_total;
    const uint32_t ex = wave_excl_scan_u32(c, &wave_total);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t wv = 0; wv < (threadIdx.x >> 6); ++wv) before += sh[wv];
    const uint32_t boff = block_off[blockIdx.x];
    unsigned long long o = J.out_off + boff + before + ex;
    const uint32_t doc0 = lo_doc + b * kDenseBlockDocs + threadIdx.x * kDensePerThread;
#pragma unroll
    for (uint32_t i = 0; i < kDensePerThread; ++i)
        if (k[i]) {
            out_docs[o] = doc0 + i;
            out_vals[o] = __uint_as_float(unorder_f32(k[i]));
            ++o;
        }
    if (b + 1u == J.n_blocks && threadIdx.x < 8u) {  // list padding, as k_union<write>
        const unsigned long long e = J.out_off + boff + (sh[0] + sh[1] + sh[2] + sh[3]) + threadIdx.x;
        out_docs[e] = 0xFFFFFFFFu;
        out_vals[e] = 0.0f;
    }
}

void launch_union_dense_scatter(hipStream_t st, const UDenseList* lists, uint32_t n_lists, uint64_t total_postings, const UDenseJob* jobs, uint32_t* slab, uint32_t lo_doc,
                                uint32_t range) {
    if (!n_lists || !total_postings) return;
    const uint64_t grid = (total_postings + kDenseTile - 1) / kDenseTile;
    hipLaunchKernelGGL(k_union_dense_scatter, dim3(uint32_t(grid)), dim3(kDenseThreads), 0, st, lists, n_lists, jobs, slab, lo_doc, range);
}
void launch_union_dense_count(hipStream_t st, const UDenseJob* jobs, uint32_t n_jobs, uint32_t n_blocks, const uint32_t* slab, uint32_t* block_cnt, uint32_t* block_max,
                              UDenseResult* results) {
    if (!n_jobs || !n_blocks) return;
    hipLaunchKernelGGL(k_union_dense_count, dim3(n_blocks), dim3(kDenseThreads), 0, st, jobs, n_jobs, slab, block_cnt, block_max);
    hipLaunchKernelGGL(k_union_dense_offsets, dim3(n_jobs), dim3(kDenseThreads), 0, st, jobs, block_cnt, block_max, results);
}
void launch_union_dense_write(hipStream_t st, const UDenseJob* jobs, uint32_t n_jobs, uint32_t n_blocks, const uint32_t* slab, const uint32_t* block_off, uint32_t lo_doc,
                              uint32_t* out_docs, float* out_vals) {
    if (!n_jobs || !n_blocks) return;
    hipLaunchKernelGGL(k_union_dense_write, dim3(n_blocks), dim3(kDenseThreads), 0, st, jobs, n_jobs, slab, block_off, lo_doc, out_docs, out_vals);
}

}  // namespace vq
