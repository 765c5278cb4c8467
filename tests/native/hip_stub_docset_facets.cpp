// TEST INFRASTRUCTURE — the launchers of veloci_amd/csrc/docset_facets.hip for the host builds that stub the device layer (see hip_stub.cpp).
// Without VQ_STUB_DICT_SCAN they throw like every other launcher.  With VQ_STUB_DICT_SCAN=1 they are answered on the host by plain loops over the
// kernel's own operands — the set's padded ids, the facet descriptors, the zeroed histogram area; the selection's jobs — so that the host side of
// the facet counts (field resolution, the layout of the call's area, the mode per facet, the device / host ranking split, the shard sum, the
// rendering, the error paths) runs end to end without a GPU.  What the kernel relies on and the host must guarantee is checked here and thrown
// when it does not hold.  Never linked into the product library.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
static void dsf_needs_host_loop(const char* what) {
    if (!std::getenv("VQ_STUB_DICT_SCAN")) throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: ") + what);
}
static void dsf_bad(const char* kernel, const char* what) { throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string(kernel) + " (stub): " + what); }

void launch_docset_facet_count(hipStream_t, const uint32_t* docs, uint32_t local_len, const DocsetFacetD* facets, uint32_t m, uint32_t* hist) {
    dsf_needs_host_loop("k_docset_facet_count");
    if (!local_len || !m) return;
    const char* k = "k_docset_facet_count";
    if (m > 65535) dsf_bad(k, "more facets than a grid has rows");
    if (reinterpret_cast<uintptr_t>(docs) & 15u) dsf_bad(k, "ids that are not 16-byte aligned");
    for (uint32_t i = 1; i < local_len; ++i)
        if (docs[i - 1] >= docs[i]) dsf_bad(k, "ids that do not ascend");
    for (uint32_t i = local_len; i < ((local_len + 3u) & ~3u); ++i)
        if (docs[i] != 0xFFFFFFFFu) dsf_bad(k, "ids without their padding");
    const char* no_lds = std::getenv("VQ_NO_DOCSET_FACET_LDS");
    const bool forced = no_lds && no_lds[0] && no_lds[0] != '0';
    for (uint32_t f = 0; f < m; ++f) {
        const DocsetFacetD& fa = facets[f];
        if (fa.lds && fa.num_values > kDocsetFacetLdsValues) dsf_bad(k, "a histogram in LDS mode that does not fit the LDS");
        if (fa.lds != ((!forced && fa.num_values <= kDocsetFacetLdsValues) ? 1u : 0u)) dsf_bad(k, "a mode the rule does not give");
        if (fa.hist_off & 3u) dsf_bad(k, "a histogram that does not start on a 16-byte boundary");
        if (f && fa.hist_off < facets[f - 1].hist_off + facets[f - 1].num_values) dsf_bad(k, "histograms that overlap");
        if (!fa.direct && fa.num_keys && !fa.offsets) dsf_bad(k, "a facet without a source");
        uint32_t* h = hist + fa.hist_off;
        for (uint32_t i = 0; i < local_len; ++i) {  // (bounded by local_len: the padding is never counted)
            const uint32_t row = docs[i] - fa.key_base;
            if (row >= fa.num_keys) continue;
            if (fa.direct) {
                const uint32_t v = fa.direct[row];
                if (v != 0xFFFFFFFFu && v < fa.num_values) ++h[v];
                continue;
            }
            if (fa.offsets[row] > fa.offsets[row + 1]) dsf_bad(k, "CSR offsets that descend");
            for (uint64_t e = fa.offsets[row]; e < fa.offsets[row + 1]; ++e)
                if (fa.values[e] < fa.num_values) ++h[fa.values[e]];
        }
    }
}

// k_facet_select / k_facet_select_wide restated: per job the top entries by (count descending, value id ascending), zero counts never reported
void launch_docset_facet_rank(hipStream_t, uint32_t n_jobs, const FacetJob* jobs, const uint32_t* hist, uint32_t* out_vals, uint32_t* out_counts, uint32_t* out_n) {
    dsf_needs_host_loop("k_facet_select");
    for (uint32_t j = 0; j < n_jobs; ++j) {
        const FacetJob& job = jobs[j];
        if (job.top > uint32_t(kMaxTopK)) dsf_bad("k_facet_select", "more entries than the kernels rank");
        const uint32_t* h = hist + job.hist_off;
        std::vector<uint32_t> order;
        for (uint32_t v = 0; v < job.num_values; ++v)
            if (h[v]) order.push_back(v);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return h[x] != h[y] ? h[x] > h[y] : x < y; });
        const uint32_t n = uint32_t(std::min<size_t>(order.size(), job.top));
        for (uint32_t i = 0; i < n; ++i) {
            out_vals[job.out_off + i] = order[i];
            out_counts[job.out_off + i] = h[order[i]];
        }
        out_n[j] = n;
    }
}
}  // namespace vq
