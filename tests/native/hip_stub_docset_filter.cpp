// TEST INFRASTRUCTURE — the launcher of veloci_amd/csrc/docset_filter.hip for the host builds that stub the device layer (see hip_stub.cpp).
// Without VQ_STUB_DICT_SCAN it throws like every other launcher.  With VQ_STUB_DICT_SCAN=1 it is answered on the host by a plain loop over whole
// bitmaps: a leaf is the union of its lists' ids (read from `docs`, whatever other images a list carries), AND / OR fold the topmost entries, the
// root goes into the scratch bitmap — so that the host side of a doc set from a filter (the filter-only compilation, the staged program, the shared
// image tail, the length on a shard, the error paths) runs end to end without a GPU.  Never linked into the product library.
#include <cstdlib>
#include <string>
#include <vector>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
void launch_docset_filter(hipStream_t, const DList* lists, uint32_t n_lists, const DOp* fops, uint32_t n_fops, uint32_t stack_depth, uint32_t doc_lo, uint32_t doc_hi,
                          uint32_t* scratch, uint64_t scratch_words) {
    if (!std::getenv("VQ_STUB_DICT_SCAN")) throw vqreq::VelociError(vqreq::ERR_DEVICE, "device layer stubbed: k_filter_bits");
    auto bad = [](const char* what) { throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("k_filter_bits (stub): ") + what); };
    if (scratch_words % 16) bad("a scratch bitmap the kernel would not take");
    std::vector<std::vector<uint32_t>> stack;
    for (uint32_t i = 0; i < n_fops; ++i) {
        const DOp& op = fops[i];
        if (op.kind == OP_LEAF) {
            if (uint32_t(op.list_begin) + op.list_count > n_lists) bad("a list the program does not have");
            std::vector<uint32_t> bits(scratch_words, 0u);
            for (uint32_t j = 0; j < op.list_count; ++j) {
                const DList& l = lists[op.list_begin + j];
                if (reinterpret_cast<uintptr_t>(l.docs) & 15u) bad("a list that is not 16-byte aligned");
                for (uint32_t e = 0; e < l.len; ++e) {
                    const uint32_t doc = l.docs[e];
                    if (doc < doc_lo || doc >= doc_hi || (e && l.docs[e - 1] >= doc)) bad("a list that is not ascending inside the shard");
                    bits[doc >> 5] |= 1u << (doc & 31u);
                }
                for (uint32_t e = l.len; e % 4; ++e)
                    if (l.docs[e] != 0xFFFFFFFFu) bad("a list without its padding");
            }
            stack.push_back(std::move(bits));
        } else {
            if ((op.kind != OP_AND && op.kind != OP_OR) || op.nchild < 1 || op.nchild > stack.size()) bad("an op the kernel would not take");
            std::vector<uint32_t>& dst = stack[stack.size() - op.nchild];
            for (uint32_t c = 1; c < op.nchild; ++c) {
                const std::vector<uint32_t>& src = stack[stack.size() - op.nchild + c];
                for (uint64_t w = 0; w < scratch_words; ++w) dst[w] = op.kind == OP_AND ? (dst[w] & src[w]) : (dst[w] | src[w]);
            }
            stack.resize(stack.size() - (op.nchild - 1u));
        }
        if (stack.size() > stack_depth) bad("a stack deeper than the launch was sized for");
    }
    if (!n_fops) return;
    if (stack.size() != 1) bad("a program that does not leave one entry");
    for (uint64_t w = 0; w < scratch_words; ++w) scratch[w] = stack[0][w];
}
}  // namespace vq
