// Doc sets: a caller's id set staged in HBM in the image the scans read for an id-only list (docs, and for the sets that qualify bitmap + rank
// directory and tile directory: the layout index.cpp builds for a posting list, see DocSet in engine.hpp).
//
// The construction goes through a scratch bitmap over ALL anchors, which sorts and de-duplicates for free.  Plain kernels in sequence on one
// stream; one wave64 per workgroup, grids capped and strided; no workgroup waits for another.
//
//   k_docset_mark     lanes stream the ids 16 B at a time over the 16-byte aligned body (up to 3 ids in front of it and behind it go one per
//                     lane) and issue a no-return atomicOr of each id's bit into the zeroed scratch bitmap.  Ids >= num_anchors set no bit: a wave
//                     counts its own with ballots and adds them to meta[0] once.
//   k_docset_count    one scratch word per lane.  Every word's popcount goes into the set's global size (meta[1], one add per wave).  A wave
//                     whose 64 words lie inside the shard's image masks the bits outside [doc_lo, doc_hi), stores the words as the local bitmap and
//                     writes the four 512-doc block counts it holds (wave_excl_scan_u32 of the popcounts, differences 16 lanes apart).
//   k_docset_scan_*   the exclusive prefix sum over the block counts, in place, as three launches: the sum of every 64 counts, one wave that scans
//                     those sums (64 per round, a carried total) and writes the closing entry, then every wave scans its 64 counts again and adds
//                     its offset.  The result is the rank directory.
//   k_docset_tiles    tile_dir[k] = rank_dir[32 k] (one entry per 16384 docs), the entries behind the image = the closing entry
//   k_docset_expand   a wave takes 64 local words: base from the rank directory, the lane's offset from the exclusive scan of the popcounts, the
//                     lane's set bits written out in ascending order.  The wave of the last words writes the 0xFFFFFFFF padding.
#include <algorithm>

#include "kernel_common.hpp"
#include "kernels.hpp"

namespace vq {

constexpr uint32_t kDocsetMaxGrid = 8192;  // workgroups of one wave; the rest of the work is strided

__global__ __launch_bounds__(64) void k_docset_mark(const uint32_t* __restrict__ ids, unsigned long long n, uint32_t num_anchors, uint32_t* __restrict__ bits,
                                                    unsigned long long* __restrict__ meta) {
    const uint32_t lane = lane_id();
    unsigned long long head = ((16u - (uint32_t)((uintptr_t)ids & 15u)) & 15u) >> 2;  // ids in front of the first 16-byte boundary
    head = head < n ? head : n;
    const unsigned long long nvec = (n - head) >> 2, tail = (n - head) & 3u;
    uint32_t bad = 0;  // (uniform: summed from ballots)
    auto mark = [&](uint32_t id, bool live) {
        const bool out = live && id >= num_anchors;
        if (live && !out) atomicOr(bits + (id >> 5), 1u << (id & 31u));
        bad += (uint32_t)__popcll(__ballot(out));
    };
    const VQ_GLOBAL u32x4* body = as_global(reinterpret_cast<const u32x4*>(ids + head));
    for (unsigned long long v0 = (unsigned long long)blockIdx.x * 64u; v0 < nvec; v0 += (unsigned long long)gridDim.x * 64u) {  // (uniform trip count)
        const unsigned long long v = v0 + lane;
        const bool live = v < nvec;
        u32x4 d = u32x4{0u, 0u, 0u, 0u};
        if (live) d = body[v];
        mark(d.x, live);
        mark(d.y, live);
        mark(d.z, live);
        mark(d.w, live);
    }
    if (blockIdx.x == 0) {
        mark(lane < head ? ids[lane] : 0u, lane < head);
        mark(lane < tail ? ids[head + nvec * 4u + lane] : 0u, lane < tail);
    }
    if (lane == 0 && bad) atomicAdd(meta, (unsigned long long)bad);
}

// scratch: scratch_words words over [0, num_anchors); the local image: `words` words (a multiple of 64) from scratch word base_word (a multiple of
// 64) on, bit 0 of its first word = doc bitmap_base.  block_counts[j / 16] = set bits of local words [16 j', 16 j' + 16) after masking.
__global__ __launch_bounds__(64) void k_docset_count(const uint32_t* __restrict__ scratch, unsigned long long scratch_words, unsigned long long base_word,
                                                     unsigned long long words, uint32_t bitmap_base, uint32_t doc_lo, uint32_t doc_hi, uint32_t* __restrict__ local,
                                                     uint32_t* __restrict__ block_counts, unsigned long long* __restrict__ meta) {
    const uint32_t lane = lane_id();
    const unsigned long long end = scratch_words > base_word + words ? scratch_words : base_word + words;
    uint32_t mine = 0;
    for (unsigned long long g0 = (unsigned long long)blockIdx.x * 64u; g0 < end; g0 += (unsigned long long)gridDim.x * 64u) {
        const unsigned long long g = g0 + lane;
        uint32_t w = g < scratch_words ? as_global(scratch)[g] : 0u;
        mine += (uint32_t)__popc(w);
        if (g0 < base_word || g0 >= base_word + words) continue;  // (uniform: both bounds are multiples of 64)
        const unsigned long long j = g - base_word;
        const unsigned long long doc0 = (unsigned long long)bitmap_base + (j << 5);
        if (doc0 + 32u <= doc_lo || doc0 >= doc_hi) w = 0u;
        else {
            if (doc0 < doc_lo) w &= 0xFFFFFFFFu << (uint32_t)(doc_lo - doc0);
            if (doc0 + 32u > doc_hi) w &= (1u << (uint32_t)(doc_hi - doc0)) - 1u;
        }
        local[j] = w;
        uint32_t total;
        const uint32_t e = wave_excl_scan_u32((uint32_t)__popc(w), &total);
        const uint32_t b = lane & 3u;
        const uint32_t lo = (uint32_t)__shfl((int)e, (int)(b * 16u));
        const uint32_t next = (uint32_t)__shfl((int)e, (int)(b == 3u ? 63u : (b + 1u) * 16u));
        if (lane < 4u) block_counts[(j >> 4) + lane] = (b == 3u ? total : next) - lo;  // (lane b < 4 holds word j0 + b: j >> 4 is the wave's first block)
    }
    uint32_t total;
    (void)wave_excl_scan_u32(mine, &total);
    if (lane == 0 && total) atomicAdd(meta + 1, (unsigned long long)total);
}

__global__ __launch_bounds__(64) void k_docset_scan_sums(const uint32_t* __restrict__ counts, unsigned long long n_parts, uint32_t* __restrict__ partials) {
    for (unsigned long long p = blockIdx.x; p < n_parts; p += gridDim.x) {
        uint32_t total;
        (void)wave_excl_scan_u32(as_global(counts)[p * 64u + lane_id()], &total);
        if (lane_id() == 0) partials[p] = total;
    }
}
// one wave: partials -> their exclusive prefix sums; closing[0] = the grand total
__global__ __launch_bounds__(64) void k_docset_scan_parts(uint32_t* __restrict__ partials, unsigned long long n_parts, uint32_t* __restrict__ closing) {
    uint32_t carry = 0;
    for (unsigned long long p0 = 0; p0 < n_parts; p0 += 64u) {
        const unsigned long long p = p0 + lane_id();
        const uint32_t x = p < n_parts ? partials[p] : 0u;
        uint32_t total;
        const uint32_t e = wave_excl_scan_u32(x, &total);
        if (p < n_parts) partials[p] = carry + e;
        carry += total;
    }
    if (lane_id() == 0) *closing = carry;
}
__global__ __launch_bounds__(64) void k_docset_scan_add(uint32_t* __restrict__ counts, unsigned long long n_parts, const uint32_t* __restrict__ partials) {
    for (unsigned long long p = blockIdx.x; p < n_parts; p += gridDim.x) {
        const unsigned long long i = p * 64u + lane_id();
        uint32_t total;
        const uint32_t e = wave_excl_scan_u32(counts[i], &total);
        counts[i] = as_global(partials)[p] + e;
    }
}
__global__ __launch_bounds__(64) void k_docset_tiles(const uint32_t* __restrict__ rank_dir, unsigned long long blocks, uint32_t* __restrict__ tile_dir, unsigned long long entries) {
    for (unsigned long long k = (unsigned long long)blockIdx.x * 64u + lane_id(); k < entries; k += (unsigned long long)gridDim.x * 64u) {
        const unsigned long long b = k << (kTileDirShift - kRankShift);
        tile_dir[k] = as_global(rank_dir)[b < blocks ? b : blocks];
    }
}

__global__ __launch_bounds__(64) void k_docset_expand(const uint32_t* __restrict__ local, const uint32_t* __restrict__ rank_dir, unsigned long long words, uint32_t bitmap_base,
                                                      uint32_t* __restrict__ docs) {
    const uint32_t lane = lane_id();
    for (unsigned long long j0 = (unsigned long long)blockIdx.x * 64u; j0 < words; j0 += (unsigned long long)gridDim.x * 64u) {
        if (j0 + 64u >= words) {  // (uniform) the wave of the last words: the padding up to a multiple of 4 entries
            const uint32_t n = as_global(rank_dir)[words >> (kRankShift - 5)];
            if (lane < ((4u - (n & 3u)) & 3u)) docs[(unsigned long long)n + lane] = 0xFFFFFFFFu;
        }
        uint32_t w = as_global(local)[j0 + lane];
        uint32_t total;
        const uint32_t e = wave_excl_scan_u32((uint32_t)__popc(w), &total);
        if (!total) continue;  // (uniform)
        unsigned long long at = (unsigned long long)as_global(rank_dir)[j0 >> (kRankShift - 5)] + e;
        const uint32_t doc0 = bitmap_base + (uint32_t)((j0 + lane) << 5);  // (a set bit lies below doc_hi: no wrap for the docs written)
        while (w) {
            docs[at++] = doc0 + (uint32_t)__builtin_ctz(w);
            w &= w - 1u;
        }
    }
}

static uint32_t docset_grid(unsigned long long waves) { return (uint32_t)(waves < 1u ? 1u : waves < kDocsetMaxGrid ? waves : kDocsetMaxGrid); }

void launch_docset_mark(hipStream_t st, const uint32_t* ids, uint64_t n, uint32_t num_anchors, uint32_t* scratch, unsigned long long* meta) {
    if (!n) return;
    hipLaunchKernelGGL(k_docset_mark, dim3(docset_grid((n / 4u + 63u) / 64u)), dim3(64), 0, st, ids, (unsigned long long)n, num_anchors, scratch, meta);
}
void launch_docset_count(hipStream_t st, const uint32_t* scratch, uint64_t scratch_words, uint64_t base_word, uint64_t words, uint32_t bitmap_base, uint32_t doc_lo,
                         uint32_t doc_hi, uint32_t* local, uint32_t* block_counts, unsigned long long* meta) {
    const uint64_t end = std::max(scratch_words, base_word + words);
    hipLaunchKernelGGL(k_docset_count, dim3(docset_grid((end + 63u) / 64u)), dim3(64), 0, st, scratch, (unsigned long long)scratch_words, (unsigned long long)base_word,
                       (unsigned long long)words, bitmap_base, doc_lo, doc_hi, local, block_counts, meta);
}
void launch_docset_scan(hipStream_t st, uint32_t* rank_dir, uint64_t blocks, uint32_t* partials) {
    const uint64_t n_parts = blocks / 64u;  // (the image is a multiple of 2048 words: blocks is a multiple of 128)
    hipLaunchKernelGGL(k_docset_scan_sums, dim3(docset_grid(n_parts)), dim3(64), 0, st, rank_dir, (unsigned long long)n_parts, partials);
    hipLaunchKernelGGL(k_docset_scan_parts, dim3(1), dim3(64), 0, st, partials, (unsigned long long)n_parts, rank_dir + blocks);
    hipLaunchKernelGGL(k_docset_scan_add, dim3(docset_grid(n_parts)), dim3(64), 0, st, rank_dir, (unsigned long long)n_parts, partials);
}
void launch_docset_tiles(hipStream_t st, const uint32_t* rank_dir, uint64_t blocks, uint32_t* tile_dir, uint64_t entries) {
    hipLaunchKernelGGL(k_docset_tiles, dim3(docset_grid((entries + 63u) / 64u)), dim3(64), 0, st, rank_dir, (unsigned long long)blocks, tile_dir, (unsigned long long)entries);
}
void launch_docset_expand(hipStream_t st, const uint32_t* local, const uint32_t* rank_dir, uint64_t words, uint32_t bitmap_base, uint32_t* docs) {
    hipLaunchKernelGGL(k_docset_expand, dim3(docset_grid(words / 64u)), dim3(64), 0, st, local, rank_dir, (unsigned long long)words, bitmap_base, docs);
}

}  // namespace vq
