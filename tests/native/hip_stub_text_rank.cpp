// TEST INFRASTRUCTURE — the launchers of veloci_amd/csrc/text_rank.hip for the host builds that stub the device layer (see hip_stub.cpp).
// Without VQ_STUB_DICT_SCAN they throw like every other launcher.  With VQ_STUB_DICT_SCAN=1 they are answered on the host by plain loops in the
// kernels' own formats — row descriptors, zero-filled `best` arrays of num_texts words per slot, (text, score bits) pairs and the two counts per
// slot — so that the host side of a highlight batch (the store check, slots, rounds, descriptor and result layout, the page's snippets) runs end
// to end without a GPU.  Never linked into the product library.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
static void text_rank_needs_host_loop(const char* what) {
    if (!std::getenv("VQ_STUB_DICT_SCAN")) throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: ") + what);
}
void launch_text_best(hipStream_t, const TextRowD* rows, uint32_t n_rows, const uint32_t* vals, uint32_t num_texts, uint32_t* best) {
    text_rank_needs_host_loop("k_text_best");
    for (uint32_t r = 0; r < n_rows; ++r) {
        if (rows[r].len > kTextRankSplit) throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_text_best (stub): a row piece longer than the split length");
        uint32_t* mine = best + size_t(rows[r].slot) * num_texts;
        for (uint32_t i = 0; i < rows[r].len; ++i) {
            const uint32_t text = vals[rows[r].start + i];
            if (text < num_texts) mine[text] = std::max(mine[text], rows[r].bits);
        }
    }
}
void launch_text_select(hipStream_t, const uint32_t* best, uint32_t num_texts, uint32_t n_slots, const uint32_t* top_ns, uint32_t out_stride, uint32_t* out_counts,
                        uint32_t* out_pairs) {
    text_rank_needs_host_loop("k_text_select");
    for (uint32_t s = 0; s < n_slots; ++s) {
        if (top_ns[s] == 0 || top_ns[s] > out_stride || out_stride > kTextRankMaxTop) throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_text_select (stub): a slot the kernel would refuse");
        std::vector<std::pair<uint32_t, uint32_t>> touched;  // (bits, text)
        for (uint32_t t = 0; t < num_texts; ++t)
            if (best[size_t(s) * num_texts + t]) touched.push_back({best[size_t(s) * num_texts + t], t});
        std::sort(touched.begin(), touched.end(), [](auto& a, auto& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
        const uint32_t n = uint32_t(std::min<size_t>(touched.size(), top_ns[s]));
        out_counts[2 * s] = n;
        out_counts[2 * s + 1] = uint32_t(touched.size());
        for (uint32_t k = 0; k < n; ++k) {  // (the kernel promises no order: written back to front)
            out_pairs[(size_t(s) * out_stride + k) * 2] = touched[n - 1 - k].second;
            out_pairs[(size_t(s) * out_stride + k) * 2 + 1] = touched[n - 1 - k].first;
        }
    }
}
}  // namespace vq
