// TEST INFRASTRUCTURE — the launchers of veloci_amd/csrc/dict_topn.hip for the host builds that stub the device layer (see hip_stub.cpp).
// Without VQ_STUB_DICT_SCAN they throw like every other launcher.  With VQ_STUB_DICT_SCAN=1 (the switch that lets hip_stub.cpp answer prefix
// probes by a plain loop) they are answered on the host in the kernels' own formats — keys rank << 32 | term, segments, class ords, buffers of
// (class << 32 | term) — by the reference's loop written out plainly, so that the host side of a suggest batch (probe ranking, descriptor and
// buffer layout, the hand-over into lookup_terms) runs end to end without a GPU.  Never linked into the product library.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
static void topn_needs_host_loop(const char* what) {
    if (!std::getenv("VQ_STUB_DICT_SCAN")) throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: ") + what);
}
size_t dict_topn_sort_tmp_bytes(uint32_t, uint32_t) { return 16; }
bool launch_dict_topn_group(hipStream_t, const DictMatch* recs, uint32_t n, const uint32_t* rank_of, uint32_t n_ranks, uint32_t n_full, unsigned long long* keys_in,
                            unsigned long long* keys_sorted, uint32_t* infos_in, uint32_t* infos_sorted, void*, size_t, uint32_t* seg) {
    topn_needs_host_loop("k_dict_topn<group>");
    std::memset(seg, 0, (2 * size_t(n_ranks) + 1) * 4);
    std::vector<std::pair<unsigned long long, uint32_t>> v(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (recs[i].probe >= n_ranks) throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_dict_topn<group> (stub): a record of a probe outside the batch");
        keys_in[i] = (static_cast<unsigned long long>(rank_of[recs[i].probe]) << 32) | recs[i].term;
        infos_in[i] = recs[i].info;
        v[i] = {keys_in[i], infos_in[i]};
    }
    std::sort(v.begin(), v.end());
    for (uint32_t i = 0; i < n; ++i) {
        keys_sorted[i] = v[i].first;
        infos_sorted[i] = v[i].second;
        const uint32_t r = uint32_t(v[i].first >> 32);
        if (i == 0 || uint32_t(v[i - 1].first >> 32) != r) seg[2 * r] = i;
        seg[2 * r + 1] = i + 1;
        if (r < n_full) seg[2 * n_ranks] = i + 1;
    }
    return true;
}
void launch_dict_topn(hipStream_t, const TopnProbeD* probes, uint32_t n_probes, uint32_t max_top_n, const unsigned long long* keys, const uint32_t* infos,
                      const uint32_t* seg, const uint16_t* class_ord, uint32_t* out_off, uint32_t* out_n, unsigned long long* out) {
    topn_needs_host_loop("k_dict_topn");
    out_off[0] = 0;
    for (uint32_t p = 0; p < n_probes; ++p) out_off[p + 1] = out_off[p] + std::min(seg[2 * probes[p].rank + 1] - seg[2 * probes[p].rank], probes[p].top_n + kTopnSlack);
    for (uint32_t p = 0; p < n_probes; ++p) {
        const TopnProbeD& P = probes[p];
        if (P.top_n == 0 || P.top_n > max_top_n || max_top_n > kTopnMax) throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_dict_topn (stub): a probe the kernel would refuse");
        std::vector<unsigned long long> buf;
        uint32_t worst = 0;
        for (uint32_t i = seg[2 * P.rank]; i < seg[2 * P.rank + 1]; ++i) {
            const uint32_t osa = infos[i] & 0xFFu, plain = (infos[i] >> 8) & 0xFFu, starts = (infos[i] >> 16) & 1u;
            const uint32_t c = 2u * (osa <= P.lev ? osa : plain) + (P.check_prefix & starts);
            const uint32_t ord = class_ord[c];
            if (ord < worst) continue;
            if (buf.size() == P.top_n + kTopnSlack) {
                std::sort(buf.begin(), buf.end(), std::greater<unsigned long long>());
                buf.resize(P.top_n);
                worst = uint32_t(buf.back() >> 41);
            }
            buf.push_back((static_cast<unsigned long long>(ord) << 41) | (static_cast<unsigned long long>(uint32_t(keys[i])) << 9) | c);
        }
        out_n[p] = uint32_t(buf.size());
        for (size_t k = 0; k < buf.size(); ++k) out[out_off[p] + k] = ((buf[k] & 0x1FFull) << 32) | ((buf[k] >> 9) & 0xFFFFFFFFull);
    }
}
int debug_dict_topn(const uint32_t*, const uint32_t*, uint32_t, uint32_t, const uint16_t*, uint32_t*, uint32_t*, uint32_t*) { return -1; }
}  // namespace vq
