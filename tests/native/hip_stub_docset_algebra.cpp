// TEST INFRASTRUCTURE — the launchers of veloci_amd/csrc/docset_algebra.hip for the host builds that stub the device layer (see hip_stub.cpp).
// Without VQ_STUB_DICT_SCAN they throw like every other launcher.  With VQ_STUB_DICT_SCAN=1 they are answered on the host by plain loops over the
// kernels' own operands — bitmap words from the index's bitmap base on, sorted padded ids — so that the host side of the set algebra (the routing,
// the rounds over a fixed operand table, the temporary bitmap, the shard masking, the error paths) runs end to end without a GPU.  What a kernel
// relies on and the host must guarantee is checked here and thrown when it does not hold.  Never linked into the product library.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
static void setop_needs_host_loop(const char* what) {
    if (!std::getenv("VQ_STUB_DICT_SCAN")) throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: ") + what);
}
static void setop_bad(const char* kernel, const char* what) { throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string(kernel) + " (stub): " + what); }
static void setop_check_ids(const char* kernel, const uint32_t* ids, uint32_t n) {
    if (reinterpret_cast<uintptr_t>(ids) & 15u) setop_bad(kernel, "ids that are not 16-byte aligned");
    for (uint32_t i = 1; i < n; ++i)
        if (ids[i - 1] >= ids[i]) setop_bad(kernel, "ids that do not ascend");
    for (uint32_t i = n; i < ((n + 3u) & ~3u); ++i)
        if (ids[i] != 0xFFFFFFFFu) setop_bad(kernel, "ids without their padding");
}

void launch_setop_words(hipStream_t, const SetOperand* ops, uint32_t n_pos, uint32_t n, bool is_or, bool init_ones, uint32_t* scratch, uint64_t scratch_words, uint64_t base_word,
                        uint64_t words, uint32_t bitmap_base, uint32_t doc_lo, uint32_t doc_hi) {
    setop_needs_host_loop("k_setop_words");
    if (n > kSetOpTable || n_pos > n) setop_bad("k_setop_words", "more operands than the table holds");
    if (words % 16 || base_word % 16 || scratch_words % 16 || (reinterpret_cast<uintptr_t>(scratch) & 15u)) setop_bad("k_setop_words", "an image the kernel would not take");
    for (uint32_t k = 0; k < n; ++k)
        if (!ops[k].bitmap || (reinterpret_cast<uintptr_t>(ops[k].bitmap) & 15u)) setop_bad("k_setop_words", "an operand without an aligned bitmap");
    if (base_word >= scratch_words) return;
    const uint64_t nw = std::min(words, scratch_words - base_word);
    for (uint64_t j = 0; j < nw; ++j) {
        uint32_t acc = scratch[base_word + j];
        if (is_or) {
            for (uint32_t k = 0; k < n; ++k) acc |= ops[k].bitmap[j];
        } else {
            if (init_ones) acc = 0xFFFFFFFFu;
            for (uint32_t k = 0; k < n_pos; ++k) acc &= ops[k].bitmap[j];
            for (uint32_t k = n_pos; k < n; ++k) acc &= ~ops[k].bitmap[j];
            for (uint32_t bit = 0; bit < 32; ++bit) {
                const uint64_t doc = uint64_t(bitmap_base) + j * 32 + bit;
                if (doc < doc_lo || doc >= doc_hi) acc &= ~(1u << bit);
            }
        }
        scratch[base_word + j] = acc;
    }
}
void launch_setop_clear(hipStream_t, const uint32_t* ids, uint32_t n, uint32_t* scratch) {
    setop_needs_host_loop("k_setop_clear");
    setop_check_ids("k_setop_clear", ids, n);
    for (uint32_t i = 0; i < n; ++i) scratch[ids[i] >> 5] &= ~(1u << (ids[i] & 31u));
}
void launch_setop_probe(hipStream_t, const uint32_t* leader, uint32_t leader_len, const SetOperand* ops, uint32_t n, bool negate, bool refine, uint32_t bitmap_base,
                        uint32_t* scratch) {
    setop_needs_host_loop("k_setop_probe");
    if (n > kSetOpTable) setop_bad("k_setop_probe", "more operands than the table holds");
    setop_check_ids("k_setop_probe", leader, leader_len);
    for (uint32_t k = 0; k < n; ++k)
        if (!ops[k].bitmap) setop_check_ids("k_setop_probe", ops[k].docs, ops[k].len);
    for (uint32_t i = 0; i < leader_len; ++i) {
        const uint32_t id = leader[i];
        if (id < bitmap_base) setop_bad("k_setop_probe", "a leader id below the bitmap base");
        bool keep = true;
        for (uint32_t k = 0; k < n && keep; ++k) {
            const uint32_t rel = id - bitmap_base;
            const bool in = ops[k].bitmap ? ((ops[k].bitmap[rel >> 5] >> (rel & 31u)) & 1u) != 0 : std::binary_search(ops[k].docs, ops[k].docs + ops[k].len, id);
            keep = in != negate;
        }
        if (!refine && keep) scratch[id >> 5] |= 1u << (id & 31u);
        if (refine && !keep) scratch[id >> 5] &= ~(1u << (id & 31u));
    }
}
}  // namespace vq
