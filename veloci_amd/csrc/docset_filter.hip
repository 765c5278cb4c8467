// Doc sets from a filter tree: the scratch bitmap over all anchors that make_docset builds its image from (docset.hip), filled by evaluating a
// filter's presence-only postfix program (CompiledQuery::fops over CompiledQuery::lists) instead of marking an id array.
//
//   k_filter_bits   one wave64 per workgroup, grid capped and strided over the tiles of 16384 docs (kTileDirShift) that [doc_lo, doc_hi) touches; a plain
//                   launch, no workgroup waits for another, no global atomics.  The evaluation stack lives in LDS: stack_depth + 1 tile bitmaps of
//                   512 words, a lane owns words [8 lane, 8 lane + 8) of every one of them (two 16-byte vectors).
//                     OP_LEAF    the union of its lists into a zeroed slot.  A LIST_BITMAP list is or-ed in from its bitmap words, 16 B per lane (the
//                                bitmap base is a multiple of 65536: a tile's words are 16-byte aligned).  Any other list is scattered from `docs`
//                                with LDS atomicOr: its in-tile range from tile_dir where the list has one, else from a wave-cooperative lower bound;
//                                lanes read 16 B each from the 4-aligned start, ids below the tile are dropped, the first id at or behind the
//                                tile's end stops the list.  A leaf without lists leaves the zeros.
//                     OP_AND/OR  over the nchild topmost slots, every lane on its own words.
//                   The root's words go out as two 16-byte stores per lane.  Lists hold only the shard's anchors, so no bit outside [doc_lo, doc_hi)
//                   is set (k_docset_count masks anyway).
#include <algorithm>

#include "kernel_common.hpp"
#include "kernels.hpp"

namespace vq {

constexpr uint32_t kFilterMaxGrid = 8192;                        // workgroups of one wave; the rest of the tiles are strided
constexpr uint32_t kFilterTileWords = 1u << (kTileDirShift - 5);  // 512 words = 2 KiB per stack slot
constexpr uint32_t kFilterTileDocs = 1u << kTileDirShift;
static_assert(kFilterTileWords == 64u * 8u, "a lane owns 8 consecutive words of a tile");

__global__ __launch_bounds__(64) void k_filter_bits(const DList* __restrict__ lists, const DOp* __restrict__ fops, uint32_t n_fops, uint32_t bitmap_base, uint32_t tile_begin,
                                                    uint32_t tile_end, uint32_t* __restrict__ scratch, unsigned long long scratch_words) {
    extern __shared__ __attribute__((aligned(16))) uint32_t filter_stack[];  // [stack_depth + 1][512]
    const uint32_t lane = lane_id();
    const VQ_CONST DOp* ops = as_const<DOp>(fops);
    const VQ_CONST DList* ls = as_const<DList>(lists);
    const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
    for (uint32_t t = tile_begin + blockIdx.x; t < tile_end; t += gridDim.x) {  // (uniform)
        const uint32_t tile_lo = t << kTileDirShift;
        const uint32_t k = t - (bitmap_base >> kTileDirShift);  // the tile's number in the lists' bitmaps and directories
        uint32_t sp = 0;
        for (uint32_t i = 0; i < n_fops; ++i) {
            const uint32_t kind = ops[i].kind;
            if (kind == OP_LEAF) {
                uint32_t* slot = filter_stack + sp * kFilterTileWords;
                u32x4* own = reinterpret_cast<u32x4*>(slot + lane * 8u);
                own[0] = zero;
                own[1] = zero;
                __syncthreads();  // (one wave: the LDS writes above are done before another lane's atomic reaches the words)
                const uint32_t lb = ops[i].list_begin, lc = ops[i].list_count;
                for (uint32_t j = 0; j < lc; ++j) {
                    const uint32_t len = ls[lb + j].len;
                    if (!len) continue;  // (uniform)
                    if (ls[lb + j].flags & LIST_BITMAP) {
                        const VQ_GLOBAL u32x4* src = as_global(reinterpret_cast<const u32x4*>(ls[lb + j].bitmap + (size_t)k * kFilterTileWords + lane * 8u));
                        const u32x4 a = src[0], b = src[1];
                        own[0] |= a;
                        own[1] |= b;
                    } else {
                        const uint32_t* docs = ls[lb + j].docs;
                        const uint32_t* tile_dir = ls[lb + j].tile_dir;
                        uint32_t start, end = len;
                        if (tile_dir) {
                            start = as_global(tile_dir)[k];
                            const uint32_t next = as_global(tile_dir)[k + 1u];
                            end = next < len ? next : len;
                        } else start = wave_lower_bound(docs, len, tile_lo);
                        const VQ_GLOBAL u32x4* vec = as_global(reinterpret_cast<const u32x4*>(docs));
                        for (uint32_t i0 = start & ~3u; i0 < end; i0 += 256u) {  // (uniform)
                            const uint32_t at = i0 + lane * 4u;
                            u32x4 d = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
                            if (at < end) d = vec[at >> 2];  // (the entries up to the next multiple of 4 exist: the list's padding)
                            bool past = false;
                            auto put = [&](uint32_t id, uint32_t idx) {
                                const uint32_t rel = id - tile_lo;
                                const bool here = idx < end && id >= tile_lo;
                                if (here && rel < kFilterTileDocs) atomicOr(slot + (rel >> 5), 1u << (rel & 31u));
                                past = past || (here && rel >= kFilterTileDocs);
                            };
                            put(d.x, at);
                            put(d.y, at + 1u);
                            put(d.z, at + 2u);
                            put(d.w, at + 3u);
                            if (__any(past)) break;  // (uniform) ascending ids: nothing of this tile follows
                        }
                    }
                    __syncthreads();  // a lane's own words are final before the next list or op reads them
                }
                ++sp;
            } else {
                const uint32_t n = ops[i].nchild;
                uint32_t* dst = filter_stack + (sp - n) * kFilterTileWords + lane * 8u;
                u32x4 a = reinterpret_cast<u32x4*>(dst)[0], b = reinterpret_cast<u32x4*>(dst)[1];
                for (uint32_t c = 1; c < n; ++c) {
                    const u32x4* src = reinterpret_cast<const u32x4*>(dst + c * kFilterTileWords);
                    if (kind == OP_AND) a &= src[0], b &= src[1];
                    else a |= src[0], b |= src[1];
                }
                reinterpret_cast<u32x4*>(dst)[0] = a;
                reinterpret_cast<u32x4*>(dst)[1] = b;
                sp -= n - 1u;
            }
        }
        // the root: slot 0 (the host checked that the program leaves exactly one entry)
        const u32x4* root = reinterpret_cast<const u32x4*>(filter_stack + lane * 8u);
        const unsigned long long w0 = (unsigned long long)t * kFilterTileWords + lane * 8u;
        u32x4* out = reinterpret_cast<u32x4*>(scratch + w0);
        if (w0 + 4u <= scratch_words) out[0] = root[0];  // (scratch_words is a multiple of 16: a vector lies inside or outside as a whole)
        if (w0 + 8u <= scratch_words) out[1] = root[1];
        __syncthreads();  // the next tile's zeroing waits for the reads above
    }
}

void launch_docset_filter(hipStream_t st, const DList* lists, uint32_t n_lists, const DOp* fops, uint32_t n_fops, uint32_t stack_depth, uint32_t doc_lo, uint32_t doc_hi,
                          uint32_t* scratch, uint64_t scratch_words) {
    (void)n_lists;
    if (!n_fops || doc_hi <= doc_lo) return;
    const uint32_t tile_begin = doc_lo >> kTileDirShift, tile_end = ((doc_hi - 1u) >> kTileDirShift) + 1u;
    const uint32_t depth = std::min<uint32_t>(std::max<uint32_t>(stack_depth, 1u), uint32_t(kStackDepth));
    const size_t lds = size_t(depth + 1u) * kFilterTileWords * 4u;
    hipLaunchKernelGGL(k_filter_bits, dim3(std::min(tile_end - tile_begin, kFilterMaxGrid)), dim3(64), lds, st, lists, fops, n_fops, doc_lo & ~65535u, tile_begin, tile_end, scratch,
                       (unsigned long long)scratch_words);
}

}  // namespace vq
