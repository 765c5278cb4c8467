// Host side of the facet counts of a doc set (docset_facets, engine.hpp): the requests resolved as a search resolves them (resolve_facet,
// compile.cpp), one zeroed histogram area and one launch of k_docset_facet_count for all facets (docset_facets.hip), then the search's own
// selection kernels for the facets they rank and the host ranking of finish_batch (exec.cpp) for the others.  On a shard the local histograms are
// downloaded, widened to u64, summed over the shards through Index::sum_over_shards and ranked on the host.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "engine.hpp"

namespace vq {

namespace {
thread_local float t_last_count_ms = -1.0f;

// count descending, value id ascending, zero counts dropped, at most `keep` entries: finish_batch's comparator, k_facet_select's order
template <class Count>
std::vector<uint32_t> rank_on_host(const Count* counts, uint32_t num_values, size_t keep) {
    std::vector<uint32_t> order;
    for (uint32_t v = 0; v < num_values; ++v)
        if (counts[v]) order.push_back(v);
    keep = std::min(keep, order.size());
    std::partial_sort(order.begin(), order.begin() + keep, order.end(), [&](uint32_t x, uint32_t y) { return counts[x] != counts[y] ? counts[x] > counts[y] : x < y; });
    order.resize(keep);
    return order;
}
}  // namespace

float docset_facets_last_count_ms() { return t_last_count_ms; }

std::unique_ptr<Result> docset_facets(const Index& idx, const DocSet& ds, const std::vector<vqreq::FacetRequest>& facets) {
    const auto t0 = std::chrono::steady_clock::now();
    t_last_count_ms = -1.0f;
    if (ds.index_uid != idx.uid) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "facet counts of a doc set: the doc set was made for another index");
    if (facets.size() > 65535) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "facet counts of a doc set: more than 65535 facets in one call");
    auto r = std::make_unique<Result>();
    r->num_hits = ds.len;
    auto stamp_time = [&] { r->execution_time_ns = uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count()); };
    if (facets.empty()) {
        stamp_time();
        return r;
    }
    std::vector<ResolvedFacet> res;
    res.reserve(facets.size());
    for (const auto& fr : facets) res.push_back(resolve_facet(idx, fr));  // (the search's own errors and declines)
    const bool sharded = idx.sharded();
    if (!idx.can_sum_over_shards())  // the counts are sums over the shards
        throw VelociError(vqreq::ERR_UNSUPPORTED, "unsupported on the MI355X query path: facet counts of a doc set on a sharded index without vq_index_set_allreduce");
    r->has_facets = true;
    const uint32_t m = uint32_t(res.size());
    auto render = [&](const ResolvedFacet& rf, ResultFacet& out, uint32_t value, uint64_t count) {
        const auto dit = idx.dict.find(rf.out.dict_path);
        std::string text = (dit != idx.dict.end() && value < dit->second.terms.size()) ? dit->second.terms[value] : std::string();
        out.entries.push_back({std::move(text), count});
    };
    for (const auto& rf : res) {
        ResultFacet f;
        f.field = rf.out.field;
        r->facets.push_back(std::move(f));
    }
    if (ds.len == 0 || (!sharded && ds.local_len == 0)) {  // nothing to count anywhere: every rank sees len == 0 and none calls the hook
        stamp_time();
        return r;
    }

    // VQ_NO_DOCSET_FACET_LDS=1 (read at every call) sends every facet through the cache mode
    const char* no_lds = std::getenv("VQ_NO_DOCSET_FACET_LDS");
    const bool lds_allowed = !(no_lds && no_lds[0] && no_lds[0] != '0');
    static const bool timing = std::getenv("VQ_DOCSET_TIMING") != nullptr;

    // the call's device area: [descriptors][jobs][histograms][out_n][out_vals][out_counts]
    std::vector<DocsetFacetD> descs(m);
    std::vector<FacetJob> jobs;         // the facets k_facet_select ranks (an unsharded index, 1 <= top <= kMaxTopK)
    std::vector<uint32_t> job_of(m, UINT32_MAX);
    uint64_t total_hist = 0;
    uint32_t total_out = 0;
    for (uint32_t i = 0; i < m; ++i) {
        const DFacet& f = res[i].f;
        DocsetFacetD& d = descs[i];
        d = DocsetFacetD{};
        d.offsets = f.offsets;
        d.values = f.values;
        d.direct = f.direct;
        d.key_base = f.key_base;
        d.num_keys = f.num_keys;
        d.num_values = f.num_values;
        d.hist_off = uint32_t(total_hist);
        d.lds = (lds_allowed && f.num_values <= kDocsetFacetLdsValues) ? 1u : 0u;
        total_hist += (uint64_t(f.num_values) + 3u) & ~uint64_t(3);  // every histogram starts on a 16-byte boundary
        if (total_hist > 0xFFFFFFFFull) throw VelociError(vqreq::ERR_UNSUPPORTED, "unsupported on the MI355X query path: facet histograms of more than 2^32 counters in one call");
        if (!sharded && f.top) {
            job_of[i] = uint32_t(jobs.size());
            jobs.push_back(FacetJob{d.hist_off, f.num_values, f.top, total_out});
            total_out += f.top;
        }
    }
    const size_t o_desc = 0, o_jobs = align_up(o_desc + m * sizeof(DocsetFacetD), 256), o_hist = align_up(o_jobs + jobs.size() * sizeof(FacetJob), 256);
    const size_t o_n = align_up(o_hist + size_t(total_hist) * 4, 256), o_vals = align_up(o_n + jobs.size() * 4, 16), o_counts = align_up(o_vals + size_t(total_out) * 4, 16);
    const size_t bytes = align_up(o_counts + size_t(total_out) * 4, 256);
    std::vector<uint8_t> up(o_hist, 0);
    std::memcpy(up.data() + o_desc, descs.data(), m * sizeof(DocsetFacetD));
    if (!jobs.empty()) std::memcpy(up.data() + o_jobs, jobs.data(), jobs.size() * sizeof(FacetJob));

    VQ_HIP(hipSetDevice(idx.device));
    const hipStream_t st = idx.pre_stream ? idx.pre_stream : idx.stream;
    DevBuf area;
    area.alloc(bytes);
    uint8_t* base = area.as<uint8_t>();
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + o_hist);
    area.upload(up.data(), up.size(), st);
    VQ_HIP(hipMemsetAsync(base + o_hist, 0, bytes - o_hist, st));
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EventGuard {
        hipEvent_t* ev;
        ~EventGuard() {
            for (int i = 0; i < 2; ++i)
                if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    } guard{ev};
    const bool timed = timing && ds.local_len;
    if (timed) {
        for (auto& e : ev) VQ_HIP(hipEventCreate(&e));
        VQ_HIP(hipEventRecord(ev[0], st));
    }
    launch_docset_facet_count(st, ds.docs.as<uint32_t>(), ds.local_len, reinterpret_cast<const DocsetFacetD*>(base + o_desc), m, hist);
    VQ_HIP(hipGetLastError());
    if (timed) VQ_HIP(hipEventRecord(ev[1], st));
    if (!jobs.empty()) {
        launch_docset_facet_rank(st, uint32_t(jobs.size()), reinterpret_cast<const FacetJob*>(base + o_jobs), hist, reinterpret_cast<uint32_t*>(base + o_vals),
                                 reinterpret_cast<uint32_t*>(base + o_counts), reinterpret_cast<uint32_t*>(base + o_n));
        VQ_HIP(hipGetLastError());
    }
    // what comes back: the selected entries, and the histograms of the facets ranked here (on a shard: of all)
    std::vector<uint8_t> down(bytes - o_n);
    std::vector<std::vector<uint32_t>> counts(m);
    if (!jobs.empty()) VQ_HIP(hipMemcpyAsync(down.data(), base + o_n, down.size(), hipMemcpyDeviceToHost, st));
    for (uint32_t i = 0; i < m; ++i)
        if (job_of[i] == UINT32_MAX && (sharded || res[i].out.host_top) && descs[i].num_values) {
            counts[i].resize(descs[i].num_values);
            VQ_HIP(hipMemcpyAsync(counts[i].data(), hist + descs[i].hist_off, size_t(descs[i].num_values) * 4, hipMemcpyDeviceToHost, st));
        }
    VQ_HIP(hipStreamSynchronize(st));
    if (timed) VQ_HIP(hipEventElapsedTime(&t_last_count_ms, ev[0], ev[1]));

    if (sharded) {  // local counts -> u64 -> one sum over the shards for the whole call -> ranked here
        std::vector<uint64_t> wide;
        for (uint32_t i = 0; i < m; ++i) wide.insert(wide.end(), counts[i].begin(), counts[i].end());
        idx.sum_over_shards(wide);
        size_t at = 0;
        for (uint32_t i = 0; i < m; ++i) {
            const uint32_t nv = uint32_t(counts[i].size());
            const size_t want = res[i].out.host_top ? res[i].out.host_top : res[i].out.top;
            for (uint32_t v : rank_on_host(wide.data() + at, nv, want)) render(res[i], r->facets[i], v, wide[at + v]);
            at += nv;
        }
        stamp_time();
        return r;
    }
    const uint32_t* out_n = reinterpret_cast<const uint32_t*>(down.data());
    const uint32_t* out_vals = reinterpret_cast<const uint32_t*>(down.data() + (o_vals - o_n));
    const uint32_t* out_counts = reinterpret_cast<const uint32_t*>(down.data() + (o_counts - o_n));
    for (uint32_t i = 0; i < m; ++i) {
        if (job_of[i] != UINT32_MAX) {
            const FacetJob& j = jobs[job_of[i]];
            for (uint32_t k = 0; k < out_n[job_of[i]] && k < j.top; ++k) render(res[i], r->facets[i], out_vals[j.out_off + k], out_counts[j.out_off + k]);
        } else if (res[i].out.host_top) {
            for (uint32_t v : rank_on_host(counts[i].data(), descs[i].num_values, res[i].out.host_top)) render(res[i], r->facets[i], v, counts[i][v]);
        }
    }
    stamp_time();
    return r;
}

}  // namespace vq
