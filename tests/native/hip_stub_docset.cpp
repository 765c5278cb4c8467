// TEST INFRASTRUCTURE — the launchers of veloci_amd/csrc/docset.hip for the host builds that stub the device layer (see hip_stub.cpp).
// Without VQ_STUB_DICT_SCAN they throw like every other launcher.  With VQ_STUB_DICT_SCAN=1 they are answered on the host by plain loops in the
// kernels' own formats — the scratch bitmap over all anchors, the masked local words with their 512-doc block counts, the rank directory scanned
// in place, the tile directory and the expanded ids with their padding — so that the host side of a doc set (buffer sizes, the layout arithmetic,
// the shard masking, the error paths, the handle's lifetime) runs end to end without a GPU.  Never linked into the product library.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
static void docset_needs_host_loop(const char* what) {
    if (!std::getenv("VQ_STUB_DICT_SCAN")) throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: ") + what);
}
void launch_docset_mark(hipStream_t, const uint32_t* ids, uint64_t n, uint32_t num_anchors, uint32_t* scratch, unsigned long long* meta) {
    docset_needs_host_loop("k_docset_mark");
    for (uint64_t i = 0; i < n; ++i) {
        if (ids[i] >= num_anchors) meta[0] += 1;
        else scratch[ids[i] >> 5] |= 1u << (ids[i] & 31u);
    }
}
void launch_docset_count(hipStream_t, const uint32_t* scratch, uint64_t scratch_words, uint64_t base_word, uint64_t words, uint32_t bitmap_base, uint32_t doc_lo,
                         uint32_t doc_hi, uint32_t* local, uint32_t* block_counts, unsigned long long* meta) {
    docset_needs_host_loop("k_docset_count");
    if (words % 64 || base_word % 64) throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_docset_count (stub): an image the kernel would not take");
    for (uint64_t g = 0; g < scratch_words; ++g) meta[1] += uint64_t(__builtin_popcount(scratch[g]));
    for (uint64_t b = 0; b < words / 16; ++b) block_counts[b] = 0;
    for (uint64_t j = 0; j < words; ++j) {
        uint32_t w = base_word + j < scratch_words ? scratch[base_word + j] : 0u;
        for (uint32_t bit = 0; bit < 32; ++bit) {
            const uint64_t doc = uint64_t(bitmap_base) + j * 32 + bit;
            if (doc < doc_lo || doc >= doc_hi) w &= ~(1u << bit);
        }
        local[j] = w;
        block_counts[j / 16] += uint32_t(__builtin_popcount(w));
    }
}
void launch_docset_scan(hipStream_t, uint32_t* rank_dir, uint64_t blocks, uint32_t*) {
    docset_needs_host_loop("k_docset_scan");
    if (blocks % 64) throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_docset_scan (stub): a block count the kernels would not take");
    uint32_t below = 0;
    for (uint64_t b = 0; b < blocks; ++b) {
        const uint32_t c = rank_dir[b];
        rank_dir[b] = below;
        below += c;
    }
    rank_dir[blocks] = below;
}
void launch_docset_tiles(hipStream_t, const uint32_t* rank_dir, uint64_t blocks, uint32_t* tile_dir, uint64_t entries) {
    docset_needs_host_loop("k_docset_tiles");
    for (uint64_t k = 0; k < entries; ++k) tile_dir[k] = rank_dir[std::min<uint64_t>(k << (kTileDirShift - kRankShift), blocks)];
}
void launch_docset_expand(hipStream_t, const uint32_t* local, const uint32_t* rank_dir, uint64_t words, uint32_t bitmap_base, uint32_t* docs) {
    docset_needs_host_loop("k_docset_expand");
    uint64_t at = 0;
    for (uint64_t j = 0; j < words; ++j) {
        if (j % 16 == 0 && rank_dir[j / 16] != at) throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_docset_expand (stub): the rank directory does not match the bitmap");
        for (uint32_t bit = 0; bit < 32; ++bit)
            if ((local[j] >> bit) & 1u) docs[at++] = uint32_t(uint64_t(bitmap_base) + j * 32 + bit);
    }
    for (; at % 4; ++at) docs[at] = 0xFFFFFFFFu;
}
}  // namespace vq
