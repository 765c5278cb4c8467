// Batch executor: compile n requests, pack their device programs, launch the kernels, assemble results.
// One batch == one k_tile_scan launch over all (query, span) pairs (SURVEY.md §7 "design for batches").
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "engine.hpp"

#include "text.hpp"

namespace vq {

using namespace vqreq;

void DevBuf::ensure(size_t n) {
    if (n <= bytes) return;
    size_t want = std::max(n, bytes + bytes / 2);
    alloc(want);
}
PinnedBuf::~PinnedBuf() {
    if (p) (void)hipHostFree(p);
}
void PinnedBuf::ensure(size_t n) {
    if (n <= bytes) return;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    size_t want = std::max(n, bytes + bytes / 2);
    VQ_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    bytes = want;
}

extern std::atomic<uint64_t> g_compile_ns[16];
static bool timing_enabled() {
    static const bool on = std::getenv("VQ_TIMING") != nullptr;
    return on;
}
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

const char* const kKernelNames[K_COUNT_] = {"k_dict_scan", "k_dict_regex", "k_dict_topn<group>", "k_dict_topn", "k_text_best", "k_text_select", "k_union<count>", "k_union<write>", "k_union_dense_scatter", "k_union_dense_count", "k_union_dense_write", "k_range_hits", "k_tile_scan<count pre-pass>", "k_scan_leaf_f32",
                                            "k_scan_simple<2,rich>", "k_scan_probe (AND / OR)", "k_scan_simple<2> (AND)", "k_scan_simple<2>", "k_scan_union", "k_scan_wide", "k_tile_scan",
                                            "k_merge_spans", "k_finalize", "k_facet_select", "k_locality", "k_boost1n"};

LaunchTimer::LaunchTimer(bool on, Workspace& w, hipStream_t s, int kernel, uint64_t layout_bytes, uint64_t algorithmic_bytes, uint64_t queries) {
    if (!on) return;
    if (w.ev_pool.empty()) {
        w.ev_pool.resize(96, nullptr);
        for (auto& e : w.ev_pool) VQ_HIP(hipEventCreate(&e));
    }
    if (w.ev_used + 2 > w.ev_pool.size()) return;  // (more launches than events: the rest of the batch goes untimed)
    ws = &w;
    st = s;
    slot = w.timed.size();
    w.timed.push_back(TimedLaunch{kernel, w.ev_used, w.ev_used + 1, layout_bytes, algorithmic_bytes, queries});
    w.ev_used += 2;
    VQ_HIP(hipEventRecord(w.ev_pool[w.timed[slot].ev_begin], st));
}
LaunchTimer::~LaunchTimer() {
    if (ws) (void)hipEventRecord(ws->ev_pool[ws->timed[slot].ev_end], st);
}

// host threads per index for request compilation (the caller counts as one): VQ_HOST_THREADS, else the machine's, at most 16 (a GPU's share of
// the host on an 8-GPU node)
size_t host_threads() {
    static const size_t n = [] {
        const char* e = std::getenv("VQ_HOST_THREADS");
        size_t hw = std::max(1u, std::thread::hardware_concurrency());
        if (const char* lws = std::getenv("LOCAL_WORLD_SIZE"); lws && std::atoi(lws) > 1)  // one process per GPU (torch.distributed.run): this rank's share of the node
            hw = std::max<size_t>(hw / size_t(std::atoi(lws)), 2);
        size_t v = e ? size_t(std::atoi(e)) : std::min<size_t>(16, hw);
        return std::min<size_t>(std::max<size_t>(v, 1), 64);
    }();
    return n;
}
// [begin, end) parts of n items for `threads` workers, shrinking: each part is 1 / (2 x threads) of what is left, at least one item
// `singles`: that many leading items are parts of their own (items sorted heaviest first: the heavy ones must not queue up behind each other)
static std::vector<std::pair<size_t, size_t>> guided_ranges(size_t n, size_t threads, size_t singles = 0) {
    std::vector<std::pair<size_t, size_t>> out;
    if (threads <= 1) {
        if (n) out.push_back({0, n});
        return out;
    }
    singles = std::min(singles, n);
    for (size_t b = 0; b < singles; ++b) out.push_back({b, b + 1});
    if (singles) {
        for (auto& r : guided_ranges(n - singles, threads)) out.push_back({r.first + singles, r.second + singles});
        return out;
    }
    static const size_t fixed = std::getenv("VQ_COMPILE_PART") ? size_t(std::atoi(std::getenv("VQ_COMPILE_PART"))) : 0;  // (experiments: parts of a fixed size)
    for (size_t b = 0; b < n;) {
        const size_t len = fixed ? std::min(fixed, n - b) : std::max<size_t>((n - b) / (2 * threads), 1);
        out.push_back({b, b + len});
        b += len;
    }
    return out;
}
static HostPool& host_pool(const Index& idx) {
    std::lock_guard<std::mutex> g(idx.pool_mu);
    if (!idx.pool) idx.pool = std::make_unique<HostPool>(host_threads() - 1);
    return *idx.pool;
}

// serialise one compiled query into `dst` (host), whose device address will be `dev`
static size_t pack_blob(const CompiledQuery& cq, const Index& idx, uint8_t* dst, const uint8_t* dev, uint32_t keys_base, uint32_t part_keys_off,
                        const std::vector<uint32_t>& hist_off, const std::vector<uint32_t>& fac_out_off, size_t* desc_bytes_out = nullptr, uint32_t stat_off = 0) {
    size_t off = align_up(sizeof(QHeader), 16);
    QHeader h{};
    auto section = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 16);
        return o;
    };
    h.n_lists = uint32_t(cq.lists.size());
    h.n_ops = uint32_t(cq.ops.size());
    h.n_fops = uint32_t(cq.fops.size());
    h.n_groups = uint32_t(cq.groups.size());
    h.n_tboost = uint32_t(cq.tboosts.size());
    h.n_col = cq.n_top_cols;
    h.n_locf = uint32_t(cq.locf.size());
    h.n_facets = uint32_t(cq.facets.size());
    h.off_lists = uint32_t(section(cq.lists.size() * sizeof(DList)));
    h.off_ops = uint32_t(section(cq.ops.size() * sizeof(DOp)));
    h.off_fops = uint32_t(section(cq.fops.size() * sizeof(DOp)));
    h.off_groups = uint32_t(section(cq.groups.size() * sizeof(DGroup)));
    h.off_tboost = uint32_t(section(cq.tboosts.size() * sizeof(DTermBoost)));
    h.off_col = uint32_t(section(cq.cols.size() * sizeof(DColBoost)));
    h.off_locf = uint32_t(section(cq.locf.size() * sizeof(DLocField)));
    h.off_facets = uint32_t(section(cq.facets.size() * sizeof(DFacet)));
    h.n_pres = uint32_t(cq.pres.size());
    h.off_pres = uint32_t(section(cq.pres.size() * sizeof(DPresOp)));
    h.off_pres_in = uint32_t(section(cq.pres_in.size() * sizeof(uint16_t)));
    h.off_loc_idx = uint32_t(section(cq.loc_idx.size() * sizeof(uint16_t)));
    h.off_simple2 = uint32_t(section(sf_rich(cq.simple_flags) ? sizeof(DSimple2) : sf_wide(cq.simple_flags) ? sizeof(DWide) : sf_probe(cq.simple_flags) || sf_union_packed(cq.simple_flags) ? sizeof(DProbe) : 0));
    const bool pool = sf_probe(cq.simple_flags) && cq.top_k <= kPoolMaxK;
    h.off_pool = pool ? uint32_t(section(sizeof(DPool) + 8 * size_t(cq.top_k))) : 0u;
    h.n_temps = cq.n_temps;
    h.n_counts = cq.n_counts;
    h.prune_n = cq.prune_n;
    h.seq_tiles = cq.seq_tiles;
    h.key_upper = cq.key_upper;
    h.prune_mask = cq.prune_mask;
    std::memcpy(h.prune_gbits, cq.prune_gbits, sizeof h.prune_gbits);
    h.simple_n = cq.simple_n;
    h.bitmap_base = idx.bitmap_base;
    h.simple_flags = cq.simple_flags;
    h.desc_bytes = uint32_t(off);
    if (desc_bytes_out) *desc_bytes_out = off;
    std::vector<size_t> inline_off(cq.inline_lists.size());
    for (size_t i = 0; i < cq.inline_lists.size(); ++i) inline_off[i] = section(align_up(cq.inline_lists[i].size(), 4) * 4);
    std::vector<size_t> inline_val_off(cq.inline_vals.size());
    for (size_t i = 0; i < cq.inline_vals.size(); ++i) inline_val_off[i] = section(align_up(cq.inline_vals[i].size(), 4) * 4);
    h.top_k = cq.top_k;
    h.tile_words = cq.tile_words;
    h.n_spans = cq.n_spans;
    h.keys_base = keys_base;
    h.doc_lo = idx.doc_lo;
    h.doc_hi = idx.doc_hi;
    h.part_keys_off = part_keys_off;
    h.stat_off = stat_off;
    h.blob_bytes = uint32_t(off);
    if (!dst) return off;

    std::memcpy(dst, &h, sizeof h);
    if (h.off_pool) std::memset(dst + h.off_pool, 0, sizeof(DPool) + 8 * size_t(cq.top_k));
    DList* dl = reinterpret_cast<DList*>(dst + h.off_lists);
    for (size_t i = 0; i < cq.lists.size(); ++i) {
        const HList& l = cq.lists[i];
        DList d{};
        d.docs = l.inline_idx >= 0 ? reinterpret_cast<const uint32_t*>(dev + inline_off[l.inline_idx]) : l.d_docs;
        d.scores = l.inline_val_idx >= 0 ? reinterpret_cast<const uint16_t*>(dev + inline_val_off[l.inline_val_idx]) : l.d_scores;
        d.len = l.len;
        d.flags = l.flags;
        d.term_score = l.term_score;
        d.max_raw = l.max_raw;
        d.pivot_raw = l.pivot_raw;
        d.bitmap = l.d_bitmap;
        d.rank_dir = l.d_rank_dir;
        d.tile_dir = l.d_tile_dir;
        dl[i] = d;
    }
    if (!cq.ops.empty()) std::memcpy(dst + h.off_ops, cq.ops.data(), cq.ops.size() * sizeof(DOp));
    if (!cq.fops.empty()) std::memcpy(dst + h.off_fops, cq.fops.data(), cq.fops.size() * sizeof(DOp));
    if (!cq.groups.empty()) std::memcpy(dst + h.off_groups, cq.groups.data(), cq.groups.size() * sizeof(DGroup));
    if (!cq.tboosts.empty()) std::memcpy(dst + h.off_tboost, cq.tboosts.data(), cq.tboosts.size() * sizeof(DTermBoost));
    if (!cq.cols.empty()) std::memcpy(dst + h.off_col, cq.cols.data(), cq.cols.size() * sizeof(DColBoost));
    if (!cq.locf.empty()) std::memcpy(dst + h.off_locf, cq.locf.data(), cq.locf.size() * sizeof(DLocField));
    if (!cq.loc_idx.empty()) std::memcpy(dst + h.off_loc_idx, cq.loc_idx.data(), cq.loc_idx.size() * sizeof(uint16_t));
    if (sf_rich(cq.simple_flags)) std::memcpy(dst + h.off_simple2, &cq.simple2, sizeof(DSimple2));
    if (sf_wide(cq.simple_flags)) std::memcpy(dst + h.off_simple2, &cq.wide, sizeof(DWide));
    if (sf_probe(cq.simple_flags) || sf_union_packed(cq.simple_flags)) std::memcpy(dst + h.off_simple2, &cq.probe, sizeof(DProbe));
    if (!cq.pres.empty()) std::memcpy(dst + h.off_pres, cq.pres.data(), cq.pres.size() * sizeof(DPresOp));
    if (!cq.pres_in.empty()) std::memcpy(dst + h.off_pres_in, cq.pres_in.data(), cq.pres_in.size() * sizeof(uint16_t));
    DFacet* df = reinterpret_cast<DFacet*>(dst + h.off_facets);
    for (size_t i = 0; i < cq.facets.size(); ++i) {
        DFacet f = cq.facets[i];
        f.hist_off = i < hist_off.size() ? hist_off[i] : 0u;  // (the count pre-pass packs queries without facet outputs)
        f.out_off = i < fac_out_off.size() ? fac_out_off[i] : 0u;
        df[i] = f;
    }
    for (size_t i = 0; i < cq.inline_vals.size(); ++i)
        if (!cq.inline_vals[i].empty()) std::memcpy(dst + inline_val_off[i], cq.inline_vals[i].data(), cq.inline_vals[i].size() * 4);
    for (size_t i = 0; i < cq.inline_lists.size(); ++i) {
        uint32_t* p = reinterpret_cast<uint32_t*>(dst + inline_off[i]);
        const auto& v = cq.inline_lists[i];
        std::memcpy(p, v.data(), v.size() * 4);
        for (size_t k = v.size(); k < align_up(v.size(), 4); ++k) p[k] = 0xFFFFFFFFu;
    }
    return off;
}

// ---- leaf top-n of a suggest batch (dict_topn.hip)
namespace {
// The 512 score classes (2 * distance + prefix_matches) as the HOST scores them: the device's log2 is not glibc's, so the kernel compares ranks of
// these floats and never a score of its own.  ord = 0xFFFF - rank among the distinct values, best first; equal floats share a rank.
struct TopnClasses {
    float score[kTopnClasses];
    uint16_t ord[kTopnClasses];
};
const TopnClasses& topn_classes() {
    static const TopnClasses table = [] {
        TopnClasses t;
        std::vector<float> distinct;
        for (uint32_t c = 0; c < kTopnClasses; ++c) distinct.push_back(t.score[c] = default_score_for_distance_host(uint8_t(c >> 1), (c & 1u) != 0));
        std::sort(distinct.begin(), distinct.end(), std::greater<float>());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        for (uint32_t c = 0; c < kTopnClasses; ++c)
            t.ord[c] = uint16_t(0xFFFFu - (std::lower_bound(distinct.begin(), distinct.end(), t.score[c], std::greater<float>()) - distinct.begin()));
        return t;
    }();
    return table;
}

}  // namespace
void topn_class_ords(uint16_t* ord) { std::memcpy(ord, topn_classes().ord, sizeof topn_classes().ord); }
namespace {
// The scans of `todo` have appended `count` records to d_recs.  Group them by probe on the device, run k_dict_topn for the top-n probes and
// fill their `matches` / `scores` with its buffers; `recs` receives the records of the other probes (probe = index into todo), and only
// those and the buffers are copied back.
void select_topn_on_device(const Index& idx, Workspace& ws, hipStream_t st, const std::vector<FuzzyProbe*>& todo, const DictMatch* d_recs, uint32_t count,
                           std::vector<DictMatch>& recs) {
    const uint32_t n_ranks = uint32_t(todo.size());
    uint32_t n_full = 0;
    for (const FuzzyProbe* fp : todo) n_full += fp->top_n == 0;
    // the full-route probes are ranked first: their records are one contiguous piece at the front of the sorted arrays
    std::vector<uint32_t> rank_of(n_ranks), probe_of(n_ranks), desc_probe;
    std::vector<TopnProbeD> descs;
    uint32_t next_full = 0, next_topn = n_full, max_top_n = 0;
    uint64_t room = 0;  // entries of all buffers when every one fills up
    for (uint32_t i = 0; i < n_ranks; ++i) {
        const FuzzyProbe& fp = *todo[i];
        rank_of[i] = fp.top_n ? next_topn++ : next_full++;
        probe_of[rank_of[i]] = i;
        if (!fp.top_n) continue;
        if (fp.top_n > kTopnMax) throw VelociError(ERR_DEVICE, "internal: a top-n probe beyond the kernel's buffer");
        descs.push_back(TopnProbeD{rank_of[i], fp.top_n, fp.lev, fp.check_prefix ? 1u : 0u, {0u, 0u, 0u, 0u}});
        desc_probe.push_back(i);
        room += fp.top_n + kTopnSlack;
        max_top_n = std::max(max_top_n, fp.top_n);
    }
    const uint32_t n_topn = uint32_t(descs.size());
    const TopnClasses& classes = topn_classes();
    // tables: [rank_of][descriptors][class ord] up, [seg: 2 * n_ranks + 1][out_off: n_topn + 1][out_n: n_topn] down
    const size_t desc_at = align_up(size_t(n_ranks) * 4, 256), ord_at = desc_at + align_up(descs.size() * sizeof(TopnProbeD), 256),
                 seg_at = ord_at + align_up(sizeof classes.ord, 256), seg_words = 2 * size_t(n_ranks) + 1, down_words = seg_words + 2 * size_t(n_topn) + 1;
    ws.d_topn_meta.ensure(seg_at + down_words * 4 + 16);
    uint8_t* meta = ws.d_topn_meta.as<uint8_t>();
    uint32_t* d_seg = reinterpret_cast<uint32_t*>(meta + seg_at);
    const size_t keys_sorted_at = align_up(size_t(count) * 8, 256), infos_at = 2 * keys_sorted_at, infos_sorted_at = infos_at + align_up(size_t(count) * 4, 256);
    ws.d_topn_sort.ensure(infos_sorted_at + size_t(count) * 4 + 16);
    uint8_t* sortb = ws.d_topn_sort.as<uint8_t>();
    unsigned long long* d_keys_sorted = reinterpret_cast<unsigned long long*>(sortb + keys_sorted_at);
    uint32_t* d_infos_sorted = reinterpret_cast<uint32_t*>(sortb + infos_sorted_at);
    const size_t tmp_bytes = dict_topn_sort_tmp_bytes(count, n_ranks);
    if (tmp_bytes == size_t(-1)) throw VelociError(ERR_DEVICE, "leaf top-n: the grouping sort's storage size");
    ws.d_topn_tmp.ensure(tmp_bytes + 16);
    ws.d_topn_out.ensure(size_t(std::min<uint64_t>(room, count)) * 8 + 16);  // (the buffers are packed: a probe gets min(its matches, top_n + 200) entries)
    VQ_HIP(hipMemcpyAsync(meta, rank_of.data(), rank_of.size() * 4, hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemcpyAsync(meta + desc_at, descs.data(), descs.size() * sizeof(TopnProbeD), hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemcpyAsync(meta + ord_at, classes.ord, sizeof classes.ord, hipMemcpyHostToDevice, st));
    {
        LaunchTimer timer(idx.profile.enabled, ws, st, K_DICT_TOPN_GROUP, uint64_t(count) * (12 + 2 * 12), uint64_t(count) * 12, n_ranks);
        if (!launch_dict_topn_group(st, d_recs, count, reinterpret_cast<const uint32_t*>(meta), n_ranks, n_full, reinterpret_cast<unsigned long long*>(sortb), d_keys_sorted,
                                    reinterpret_cast<uint32_t*>(sortb + infos_at), d_infos_sorted, ws.d_topn_tmp.p, tmp_bytes, d_seg))
            throw VelociError(ERR_DEVICE, "leaf top-n: the grouping sort could not be queued");
    }
    {
        LaunchTimer timer(idx.profile.enabled, ws, st, K_DICT_TOPN, 0, 0, n_topn);
        launch_dict_topn(st, reinterpret_cast<const TopnProbeD*>(meta + desc_at), n_topn, max_top_n, d_keys_sorted, d_infos_sorted, d_seg,
                         reinterpret_cast<const uint16_t*>(meta + ord_at), d_seg + seg_words, d_seg + seg_words + n_topn + 1, ws.d_topn_out.as<unsigned long long>());
    }
    VQ_HIP(hipGetLastError());
    std::vector<uint32_t> down(down_words);
    VQ_HIP(hipMemcpyAsync(down.data(), d_seg, down_words * 4, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    const uint32_t full_records = down[seg_words - 1];
    const uint32_t* out_off = down.data() + seg_words;
    const uint32_t* out_n = out_off + n_topn + 1;
    if (full_records > count || out_off[n_topn] > count - full_records) throw VelociError(ERR_DEVICE, "leaf top-n: more records to copy back than there are");
    std::vector<unsigned long long> bufs(out_off[n_topn]), keys(full_records);
    std::vector<uint32_t> infos(full_records);
    if (!bufs.empty()) VQ_HIP(hipMemcpyAsync(bufs.data(), ws.d_topn_out.p, bufs.size() * 8, hipMemcpyDeviceToHost, st));
    if (full_records) {
        VQ_HIP(hipMemcpyAsync(keys.data(), d_keys_sorted, size_t(full_records) * 8, hipMemcpyDeviceToHost, st));
        VQ_HIP(hipMemcpyAsync(infos.data(), d_infos_sorted, size_t(full_records) * 4, hipMemcpyDeviceToHost, st));
    }
    VQ_HIP(hipStreamSynchronize(st));
    recs.resize(full_records);
    if (full_records) {
        for (uint32_t r = 0; r < full_records; ++r) {
            const uint32_t rank = uint32_t(keys[r] >> 32);
            if (rank >= n_full) throw VelociError(ERR_DEVICE, "leaf top-n: a top-n probe's record inside the full-route piece");
            recs[r] = DictMatch{probe_of[rank], uint32_t(keys[r]), infos[r]};
        }
    }
    for (uint32_t j = 0; j < n_topn; ++j) {
        FuzzyProbe& fp = *todo[desc_probe[j]];
        const uint32_t n = out_n[j];
        if (n > out_off[j + 1] - out_off[j]) throw VelociError(ERR_DEVICE, "leaf top-n: a buffer longer than its room");
        fp.topn_copied = out_off[j + 1] - out_off[j];
        fp.matches.resize(n);
        fp.scores.resize(n);
        for (uint32_t k = 0; k < n; ++k) {  // buffer order, NOT ascending ids
            const unsigned long long e = bufs[out_off[j] + k];
            fp.matches[k] = uint32_t(e);
            fp.scores[k] = classes.score[(e >> 32) & (kTopnClasses - 1u)];
        }
        fp.answered = true;
    }
}
}  // namespace

// Answer every dictionary scan of a batch with k_dict_scan launches (grid.y = probe), then bring the match
// sets back sorted ascending (== FST stream order, which is what the reference's callback order is).
void run_fuzzy_probes(const Index& idx, Workspace& ws, FuzzyTable& table, hipStream_t st) {
    std::vector<FuzzyProbe*> todo;
    for (auto& kv : table)
        if (kv.second.status == 0) todo.push_back(&kv.second);
    if (todo.empty()) return;
    auto image_of = [&](const FuzzyProbe& fp) -> const void* {  // the dictionary image a probe scans (a regex probe: always the raw one)
        const Dictionary& d = idx.dict.at(fp.path);
        return fp.ci && !fp.regex ? d.d_low.p : d.d_raw.p;
    };
    auto small_tables = [&](const FuzzyProbe& fp) {  // a regex probe whose tables fit the small form of k_dict_regex
        const Dictionary& d = idx.dict.at(fp.path);
        return vqregex::lds_table_bytes(fp.dfa.n_states, fp.dfa.n_classes, d.alphabet.size() - d.alphabet_ascii) <= vqregex::kLdsTableBytesSmall;
    };
    // k_dict_scan takes a 16-bit image and a query of <= 64 code points below U+10000 inline; every other probe goes to k_dict_scan_wide, with
    // its code points as u32 in a side pool
    auto pooled = [&](const FuzzyProbe& fp) {
        bool wide = idx.dict.at(fp.path).char_bytes != 2 || fp.query.size() > 64;
        for (uint32_t cp : fp.query) wide = wide || cp > 0xFFFFu;
        return wide;
    };
    // probes of one image (and form) next to each other: a launch scans ONE image for a run of probes (blocks answer 16 probes per pass over their terms)
    // the regex probes behind the others, those of one dictionary and one table size next to each other: todo[n_scan ..) go to k_dict_regex
    std::stable_sort(todo.begin(), todo.end(), [&](const FuzzyProbe* a, const FuzzyProbe* b) {
        if (a->regex != b->regex) return b->regex;
        const void *ia = image_of(*a), *ib = image_of(*b);
        if (a->regex) return ia != ib ? ia < ib : small_tables(*a) > small_tables(*b);
        return ia != ib ? ia < ib : pooled(*a) < pooled(*b);
    });
    size_t n_scan = 0;
    while (n_scan < todo.size() && !todo[n_scan]->regex) ++n_scan;
    std::vector<DictProbe> probes(n_scan);
    std::vector<DictProbeW> wprobes;  // indexed like `probes` (only the pooled ones are filled in); empty when no probe is pooled
    std::vector<uint32_t> pool;
    std::vector<uint8_t> host_scored(todo.size(), 0), is_pooled(todo.size(), 0);
    for (size_t i = 0; i < n_scan; ++i) {
        const FuzzyProbe& fp = *todo[i];
        const auto lcps = vqtext::decode_utf8(fp.lower_term);  // scoring side: the lower-cased term as a whole (search_field.rs:298-300)
        if (pooled(fp)) {
            if (wprobes.empty()) wprobes.resize(n_scan);
            is_pooled[i] = 1;
            DictProbeW& W = wprobes[i];
            std::memset(&W, 0, sizeof W);
            W.m = uint32_t(fp.query.size());
            W.max_d = fp.max_d;
            W.flags = (fp.transposition ? 1u : 0u) | (fp.prefix ? 2u : 0u);
            W.q_off = uint32_t(pool.size());
            pool.insert(pool.end(), fp.query.begin(), fp.query.end());
            // the device scores a hit with a bit-vector over the lower-cased term in one 64-bit word: longer ones are scored on the host
            if (lcps.size() <= 64 && idx.dict.at(fp.path).low_exact) {
                W.lm = uint32_t(lcps.size());
                W.lq_off = uint32_t(pool.size());
                pool.insert(pool.end(), lcps.begin(), lcps.end());
                if (fp.ci && lcps == fp.query) W.flags |= 4u;  // (then m <= 64: the whole query is staged in LDS)
            } else {
                W.lm = 0xFFFFFFFFu;
                host_scored[i] = 1;
            }
            continue;
        }
        DictProbe& P = probes[i];
        std::memset(&P, 0, sizeof P);
        P.m = uint32_t(fp.query.size());
        P.max_d = fp.max_d;
        P.flags = (fp.transposition ? 1u : 0u) | (fp.prefix ? 2u : 0u);
        for (size_t j = 0; j < fp.query.size(); ++j) P.query[j] = uint16_t(fp.query[j]);  // (all below U+10000: not pooled)
        bool bmp = lcps.size() <= 64 && idx.dict.at(fp.path).low_exact;
        for (uint32_t cp : lcps) bmp = bmp && cp <= 0xFFFFu;
        if (bmp) {
            P.lm = uint32_t(lcps.size());
            for (size_t j = 0; j < lcps.size(); ++j) P.lquery[j] = uint16_t(lcps[j]);
            // a case-insensitive scan matches with the very string it scores with, over the very image: the kernel then scores a hit from the
            // tables it already holds in LDS instead of re-reading the probe from HBM character by character
            bool same = fp.ci && lcps.size() == fp.query.size();
            for (size_t j = 0; same && j < lcps.size(); ++j) same = lcps[j] == fp.query[j];
            if (same) P.flags |= 4u;
        } else {
            P.lm = 0xFFFFFFFFu;
            host_scored[i] = 1;
        }
    }
    bool any_topn = false;
    for (size_t i = 0; i < todo.size(); ++i) {
        any_topn = any_topn || todo[i]->top_n != 0;
        if (todo[i]->top_n && (todo[i]->regex || host_scored[i])) throw VelociError(ERR_DEVICE, "internal: a top-n probe whose hits the device does not score");
    }
    DevBuf &d_probes = ws.d_probe_desc, &d_count = ws.d_probe_counts, &d_out = ws.d_probe_ids;
    // one descriptor buffer: [DictProbe x N][DictProbeW x N][pool]
    const size_t w_at = align_up(probes.size() * sizeof(DictProbe), 256), pool_at = w_at + align_up(wprobes.size() * sizeof(DictProbeW), 256);
    d_probes.ensure(pool_at + pool.size() * 4 + 16);
    d_count.ensure(64);
    // regex probes: [RegexProbeD x n][pool: every probe's tables in the kernel's format]
    std::vector<RegexProbeD> rprobes;
    std::vector<uint16_t> rpool;
    for (size_t i = n_scan; i < todo.size(); ++i) {
        const FuzzyProbe& fp = *todo[i];
        const Dictionary& d = idx.dict.at(fp.path);
        const vqregex::Dfa& A = fp.dfa;
        const uint32_t C = A.n_classes, n_next = A.n_states * C, n_alpha = uint32_t(d.alphabet.size()) - d.alphabet_ascii;
        RegexProbeD R{uint32_t(rpool.size()), n_next, A.start * C, A.first_accept * C};
        rprobes.push_back(R);
        const size_t end = rpool.size() + regex_words16(n_next, n_alpha);
        for (uint16_t to : A.next) rpool.push_back(uint16_t(to * C));
        uint16_t ascii[128] = {};
        for (uint32_t k = 0; k < d.alphabet_ascii; ++k) ascii[d.alphabet[k]] = A.cls[k];
        rpool.insert(rpool.end(), ascii, ascii + 128);
        rpool.insert(rpool.end(), A.cls.begin() + d.alphabet_ascii, A.cls.end());
        rpool.resize(end, uint16_t(0));
    }
    const size_t rpool_at = align_up(rprobes.size() * sizeof(RegexProbeD), 256);
    if (!rprobes.empty()) {
        ws.d_regex_tabs.ensure(rpool_at + rpool.size() * 2 + 16);
        VQ_HIP(hipMemcpyAsync(ws.d_regex_tabs.p, rprobes.data(), rprobes.size() * sizeof(RegexProbeD), hipMemcpyHostToDevice, st));
        VQ_HIP(hipMemcpyAsync(ws.d_regex_tabs.as<uint8_t>() + rpool_at, rpool.data(), rpool.size() * 2, hipMemcpyHostToDevice, st));
    }
    if (n_scan) VQ_HIP(hipMemcpyAsync(d_probes.p, probes.data(), probes.size() * sizeof(DictProbe), hipMemcpyHostToDevice, st));
    if (!wprobes.empty()) {
        VQ_HIP(hipMemcpyAsync(d_probes.as<uint8_t>() + w_at, wprobes.data(), wprobes.size() * sizeof(DictProbeW), hipMemcpyHostToDevice, st));
        if (!pool.empty()) VQ_HIP(hipMemcpyAsync(d_probes.as<uint8_t>() + pool_at, pool.data(), pool.size() * 4, hipMemcpyHostToDevice, st));
    }
    uint32_t cap = uint32_t(std::max<size_t>(64 * todo.size(), 1u << 16));  // matches of the whole batch share one output array
    std::vector<DictMatch> recs;
    for (int pass = 0; pass < 2; ++pass) {  // pass 1 only when the matches outgrew the first guess (the count is exact then)
        d_out.ensure(size_t(cap) * sizeof(DictMatch) + 16);
        VQ_HIP(hipMemsetAsync(d_count.p, 0, 4, st));
        if (n_scan) {
            uint64_t dict_bytes = 0, layout = 0;  // every probe reads its dictionary once (offsets + code points) ...
            for (size_t i = 0; i < n_scan; ++i) {
                const Dictionary& d = idx.dict.at(todo[i]->path);
                dict_bytes += d.d_off.bytes + d.d_low.bytes;
            }
            LaunchTimer timer(idx.profile.enabled, ws, st, K_DICT_SCAN, 0, dict_bytes, n_scan);
            for (size_t g0 = 0; g0 < n_scan;) {  // one launch per run of probes over the same image
                size_t g1 = g0 + 1;
                while (g1 < n_scan && image_of(*todo[g1]) == image_of(*todo[g0]) && is_pooled[g1] == is_pooled[g0]) ++g1;
                const Dictionary& d = idx.dict.at(todo[g0]->path);
                if (is_pooled[g0])
                    launch_dict_scan_wide(st, d.char_bytes, reinterpret_cast<const DictProbeW*>(d_probes.as<uint8_t>() + w_at) + g0,
                                          reinterpret_cast<const uint32_t*>(d_probes.as<uint8_t>() + pool_at), uint32_t(g0), uint32_t(g1 - g0), d.d_off.as<uint32_t>(),
                                          image_of(*todo[g0]), d.d_low.p, uint32_t(d.terms.size()), d_count.as<uint32_t>(), cap, d_out.as<DictMatch>());
                else
                    launch_dict_scan(st, d_probes.as<DictProbe>() + g0, uint32_t(g0), uint32_t(g1 - g0), d.d_off.as<uint32_t>(),
                                     static_cast<const uint16_t*>(image_of(*todo[g0])), d.d_low.as<uint16_t>(), uint32_t(d.terms.size()), d_count.as<uint32_t>(), cap,
                                     d_out.as<DictMatch>());
                layout += (d.d_off.bytes + d.d_low.bytes) * ((g1 - g0 + 15) / 16);  // ... this layout: once per 16 probes of one image
                g0 = g1;
            }
            if (!ws.timed.empty() && idx.profile.enabled) ws.timed.back().layout_bytes = layout;
        }
        if (n_scan < todo.size()) {  // k_dict_regex: grid.y = probe, every probe reads its dictionary's offsets and raw image (and its own tables)
            uint64_t dict_bytes = 0;
            for (size_t i = n_scan; i < todo.size(); ++i) {
                const Dictionary& d = idx.dict.at(todo[i]->path);
                dict_bytes += d.d_off.bytes + d.d_raw.bytes;
            }
            LaunchTimer timer(idx.profile.enabled, ws, st, K_DICT_REGEX, dict_bytes + rpool.size() * 2, dict_bytes, todo.size() - n_scan);
            for (size_t g0 = n_scan; g0 < todo.size();) {  // one launch per run of probes over one dictionary with tables of one size class
                size_t g1 = g0 + 1;
                const bool small = small_tables(*todo[g0]);
                while (g1 < todo.size() && image_of(*todo[g1]) == image_of(*todo[g0]) && small_tables(*todo[g1]) == small) ++g1;
                const Dictionary& d = idx.dict.at(todo[g0]->path);
                launch_dict_regex(st, d.char_bytes, small, ws.d_regex_tabs.as<RegexProbeD>() + (g0 - n_scan),
                                  reinterpret_cast<const uint16_t*>(ws.d_regex_tabs.as<uint8_t>() + rpool_at), d.d_alpha.as<uint32_t>(),
                                  uint32_t(d.alphabet.size()) - d.alphabet_ascii, uint32_t(g0), uint32_t(g1 - g0), d.d_off.as<uint32_t>(), d.d_raw.p,
                                  uint32_t(d.terms.size()), d_count.as<uint32_t>(), cap, d_out.as<DictMatch>());
                g0 = g1;
            }
        }
        VQ_HIP(hipGetLastError());
        uint32_t count = 0;
        VQ_HIP(hipMemcpyAsync(&count, d_count.p, 4, hipMemcpyDeviceToHost, st));
        VQ_HIP(hipStreamSynchronize(st));
        if (count > cap) {
            if (pass == 1) throw VelociError(ERR_DEVICE, "dictionary scan: match count changed between passes");
            cap = count;
            continue;
        }
        if (std::getenv("VQ_TIMING")) {
            std::fprintf(stderr, "[vq timing] dictionary scan: %zu probes, %u matches\n", todo.size(), count);
        }
        if (any_topn) {  // suggest batch: only the full-route probes' records and the top-n buffers come back
            select_topn_on_device(idx, ws, st, todo, d_out.as<DictMatch>(), count, recs);
            break;
        }
        recs.resize(count);
        if (count) {
            VQ_HIP(hipMemcpyAsync(recs.data(), d_out.p, size_t(count) * sizeof(DictMatch), hipMemcpyDeviceToHost, st));
            VQ_HIP(hipStreamSynchronize(st));
        }
        break;
    }
    if (std::getenv("VQ_TIMING")) {  // the distribution of matches over the probes (a few short probes can hold most of them)
        std::vector<uint32_t> per(todo.size(), 0);
        for (auto& r : recs) per[r.probe]++;
        std::vector<uint32_t> sorted = per;
        std::sort(sorted.begin(), sorted.end(), std::greater<uint32_t>());
        std::string top;
        for (size_t i = 0; i < sorted.size() && i < 8; ++i) top += " " + std::to_string(sorted[i]);
        std::fprintf(stderr, "[vq timing] dictionary scan: most matches per probe:%s\n", top.c_str());
    }
    // bucket by probe, ascending term ids (== FST stream order, which is the reference's callback order)
    std::sort(recs.begin(), recs.end(), [](const DictMatch& a, const DictMatch& b) { return a.probe != b.probe ? a.probe < b.probe : a.term < b.term; });
    size_t r = 0;
    for (size_t i = 0; i < todo.size(); ++i) {
        FuzzyProbe& fp = *todo[i];
        if (fp.top_n) continue;  // (filled by select_topn_on_device; no record of `recs` is its)
        fp.matches.clear();
        fp.scores.clear();
        fp.answered = true;
        if (fp.regex) {  // the match set only: regex hits are scored by the compiler's host branch
            for (; r < recs.size() && recs[r].probe == i; ++r) fp.matches.push_back(recs[r].term);
            continue;
        }
        const Dictionary& dict = idx.dict.at(fp.path);
        for (; r < recs.size() && recs[r].probe == i; ++r) {
            fp.matches.push_back(recs[r].term);
            if (host_scored[i]) continue;
            const uint32_t osa = recs[r].info & 0xFFu, lev = (recs[r].info >> 8) & 0xFFu;
            const bool starts = (recs[r].info >> 16) & 1u;
            uint32_t d;
            if (osa <= fp.lev && osa < 255u) d = osa;  // the scoring automaton's answer (search_field.rs:691-702)
            else {  // its fallback, plain Levenshtein in u8 — 255 for strings of 255 bytes or more (:705-732)
                const bool long_strings = fp.lower_term.size() >= 255 || (dict.terms[recs[r].term].size() >= 200 && vqtext::to_lower_utf8(dict.terms[recs[r].term]).size() >= 255);
                d = long_strings ? 255u : lev;
                if (!long_strings && (osa == 255u || lev == 255u)) {  // capped on the device: exact on the host (never for dictionary-sized terms)
                    host_scored[i] = 2;
                    break;
                }
            }
            fp.scores.push_back(default_score_for_distance_host(uint8_t(d), fp.check_prefix && starts));
        }
        if (host_scored[i] == 2) {  // (rare) finish the bucket, then score all of it on the host
            fp.matches.clear();
            size_t r0 = r;
            while (r0 > 0 && recs[r0 - 1].probe == i) --r0;
            for (r = r0; r < recs.size() && recs[r].probe == i; ++r) fp.matches.push_back(recs[r].term);
        }
        if (host_scored[i]) score_fuzzy_probe(idx, fp);
    }
}

// K2: run the union jobs of a batch.  Level 1 merges groups of <= 64 posting lists (one lane per list); a job with
// more lists gets a level-2 task over the level-1 outputs.  Each level: count pass -> host prefix sums -> write pass.
// A job with more lists than two levels take (VQ_UNION_DENSE_MIN, 4096) goes to the dense route instead (run_union_dense).
namespace {
struct UnionTaskH {
    std::vector<UList> lists;
    UnionJob* job = nullptr;   // level 1: set when this task IS the job's result (<= 64 lists); level 2: always
    size_t parent = SIZE_MAX;  // level 1: index of the level-2 task that consumes this output
    uint64_t out_off = 0;
    uint32_t len = 0;
    float max_value = std::numeric_limits<float>::infinity();
};

void run_union_level(bool timed, Workspace& ws, std::vector<UnionTaskH>& tasks, DevBuf& docs, DevBuf& vals, DevBuf& maxes, DevBuf& meta, hipStream_t st) {
    if (tasks.empty()) return;
    std::vector<UList> ulists;
    std::vector<UTask> utasks;
    std::vector<uint32_t> span_task;
    for (size_t t = 0; t < tasks.size(); ++t) {
        UTask u{};
        u.list_begin = uint32_t(ulists.size());
        u.n_lists = uint32_t(tasks[t].lists.size());
        uint64_t total = 0;
        uint32_t piv = 0;
        for (uint32_t i = 0; i < u.n_lists; ++i) {
            total += tasks[t].lists[i].len;
            if (tasks[t].lists[i].len > tasks[t].lists[piv].len) piv = i;
            ulists.push_back(tasks[t].lists[i]);
        }
        u.pivot = u.list_begin + piv;
        static const uint64_t span_len = std::getenv("VQ_UNION_SPAN") ? std::max(1, std::atoi(std::getenv("VQ_UNION_SPAN"))) : 128;  // (bench_jmdict shape: 512 -> 36.6 k, 256 -> 43.8 k, 128 -> 44.2 k, 64 -> 45.3 k requests/s)
        uint64_t spans = std::min<uint64_t>(std::max<uint64_t>(total / span_len, 1), 4096);  // (short spans: a span is one serial merge loop, its length is the pass's latency)
        spans = std::min<uint64_t>(spans, std::max<uint32_t>(tasks[t].lists[piv].len, 1u));
        u.span_begin = uint32_t(span_task.size());
        u.n_spans = uint32_t(spans);
        for (uint32_t k = 0; k < u.n_spans; ++k) span_task.push_back(uint32_t(t));
        utasks.push_back(u);
    }
    const size_t n_spans = span_task.size();
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_lists = 0, o_tasks = al(ulists.size() * sizeof(UList)), o_st = o_tasks + al(utasks.size() * sizeof(UTask)),
                 o_cnt = o_st + al(n_spans * 4), o_off = o_cnt + al(n_spans * 4), bytes = o_off + al(n_spans * 8);
    meta.ensure(bytes);
    uint8_t* m = meta.as<uint8_t>();
    VQ_HIP(hipMemcpyAsync(m + o_lists, ulists.data(), ulists.size() * sizeof(UList), hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemcpyAsync(m + o_tasks, utasks.data(), utasks.size() * sizeof(UTask), hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemcpyAsync(m + o_st, span_task.data(), n_spans * 4, hipMemcpyHostToDevice, st));
    uint64_t in_bytes = 0;
    for (auto& u : ulists) in_bytes += uint64_t(u.len) * ((u.flags & 1u) ? 8u : 6u);
    uint64_t out_bytes = 0;
    auto launch = [&](bool write) {
        LaunchTimer timer(timed, ws, st, write ? K_UNION_WRITE : K_UNION_COUNT, in_bytes + (write ? out_bytes : 0), in_bytes + (write ? out_bytes : 0), tasks.size());
        launch_union(st, write, uint32_t(n_spans), reinterpret_cast<const UList*>(m + o_lists), reinterpret_cast<const UTask*>(m + o_tasks),
                     reinterpret_cast<const uint32_t*>(m + o_st), reinterpret_cast<uint32_t*>(m + o_cnt), reinterpret_cast<const uint64_t*>(m + o_off),
                     docs.as<uint32_t>(), vals.as<float>(), maxes.as<uint32_t>());
        VQ_HIP(hipGetLastError());
    };
    launch(false);
    std::vector<uint32_t> cnt(n_spans);
    VQ_HIP(hipMemcpyAsync(cnt.data(), m + o_cnt, n_spans * 4, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    std::vector<uint64_t> off(n_spans);
    uint64_t cursor = 0;
    for (size_t t = 0; t < tasks.size(); ++t) {
        tasks[t].out_off = cursor;
        uint64_t len = 0;
        for (uint32_t k = 0; k < utasks[t].n_spans; ++k) {
            off[utasks[t].span_begin + k] = cursor + len;
            len += cnt[utasks[t].span_begin + k];
        }
        if (len > 0xFFFFFFF0ull) throw VelociError(ERR_UNSUPPORTED, "materialised leaf longer than 2^32 entries");
        tasks[t].len = uint32_t(len);
        cursor += (len + 8 + 3) / 4 * 4;  // 8 sentinel entries behind every list, starts stay 16-byte aligned
    }
    out_bytes = cursor * 8;
    docs.ensure(cursor * 4 + 64);
    vals.ensure(cursor * 4 + 64);
    maxes.ensure(tasks.size() * 4 + 64);
    VQ_HIP(hipMemsetAsync(maxes.p, 0xFF, tasks.size() * 4, st));  // min(~order(value)) per task, written by the write pass
    VQ_HIP(hipMemcpyAsync(m + o_off, off.data(), n_spans * 8, hipMemcpyHostToDevice, st));
    launch(true);
    // the largest value of every merged list: the compiler's score bounds need it (top-k pruning of the scan)
    std::vector<uint32_t> mins(tasks.size());
    VQ_HIP(hipMemcpyAsync(mins.data(), maxes.p, tasks.size() * 4, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    for (size_t t = 0; t < tasks.size(); ++t)
        if (mins[t] != 0xFFFFFFFFu) {
            const uint32_t bits = unorder_f32(~mins[t]);
            std::memcpy(&tasks[t].max_value, &bits, 4);
        } else tasks[t].max_value = 0.0f;
}
}  // namespace

// Range jobs (k_range_hits): the leaf's postings at and between the entry anchors of its 1:n boost list; summed over the shards.
void run_range_jobs(const Index& idx, Workspace& ws, RangeTable& table, const UnionTable& unions, hipStream_t st) {
    std::vector<UList> ulists;
    std::vector<RangeJobD> jobs;
    size_t n_anchors = 0;
    uint32_t n_blocks = 0;
    for (auto& kv : table) n_anchors += kv.second.anchors ? kv.second.anchors->size() : 0;
    if (n_anchors > 0x7FFFFFF0ull) throw VelociError(ERR_UNSUPPORTED, "1:n field boosts of one batch with more than 2^31 boosted anchors");
    std::vector<uint32_t> anchors;
    anchors.reserve(n_anchors);
    for (auto& kv : table) {
        RangeJob& job = kv.second;
        const PostingStore& ps = idx.postings.at(job.store_path);
        const uint32_t lb = uint32_t(ulists.size());
        auto uit = job.union_key.empty() ? unions.end() : unions.find(job.union_key);
        if (uit != unions.end()) {  // the leaf was materialised: its merged list holds exactly the leaf's hits
            if (uit->second.len) {
                UList u{};
                u.docs = uit->second.d_docs;
                u.len = uit->second.len;
                ulists.push_back(u);
            }
        } else
        for (uint32_t tid : job.tokens) {
            if (tid >= ps.len.size() || !ps.len[tid]) continue;
            UList u{};
            u.docs = ps.docs.as<uint32_t>() + ps.start[tid];
            u.len = ps.len[tid];
            ulists.push_back(u);
        }
        RangeJobD d{};
        d.list_begin = lb;
        d.n_lists = uint32_t(ulists.size()) - lb;
        d.anchor_begin = uint32_t(anchors.size());
        d.n_anchors = job.anchors ? uint32_t(job.anchors->size()) : 0u;
        d.block_begin = n_blocks;
        if (job.anchors) anchors.insert(anchors.end(), job.anchors->begin(), job.anchors->end());
        if (d.n_lists == 0 || d.n_anchors == 0) continue;  // nothing to count: the job's counts stay 0
        n_blocks += d.n_lists == 1 ? (d.n_anchors + 63u) / 64u : d.n_anchors;
        jobs.push_back(d);
    }
    std::vector<uint64_t> counts(2 * n_anchors, 0);
    if (!jobs.empty()) {
        auto al = [](size_t x) { return (x + 255) / 256 * 256; };
        const size_t o_jobs = al(ulists.size() * sizeof(UList)), o_anchors = o_jobs + al(jobs.size() * sizeof(RangeJobD)), o_cnt = o_anchors + al(anchors.size() * 4),
                     bytes = o_cnt + al(counts.size() * 8);
        ws.d_union_meta.ensure(bytes);
        uint8_t* m = ws.d_union_meta.as<uint8_t>();
        VQ_HIP(hipMemcpyAsync(m, ulists.data(), ulists.size() * sizeof(UList), hipMemcpyHostToDevice, st));
        VQ_HIP(hipMemcpyAsync(m + o_jobs, jobs.data(), jobs.size() * sizeof(RangeJobD), hipMemcpyHostToDevice, st));
        VQ_HIP(hipMemcpyAsync(m + o_anchors, anchors.data(), anchors.size() * 4, hipMemcpyHostToDevice, st));
        VQ_HIP(hipMemsetAsync(m + o_cnt, 0, counts.size() * 8, st));
        {
            LaunchTimer timer(idx.profile.enabled, ws, st, K_RANGE_HITS, 0, 0, jobs.size());
            launch_range_hits(st, n_blocks, uint32_t(jobs.size()), reinterpret_cast<const UList*>(m), reinterpret_cast<const RangeJobD*>(m + o_jobs),
                              reinterpret_cast<const uint32_t*>(m + o_anchors), reinterpret_cast<unsigned long long*>(m + o_cnt));
        }
        VQ_HIP(hipGetLastError());
        VQ_HIP(hipMemcpyAsync(counts.data(), m + o_cnt, counts.size() * 8, hipMemcpyDeviceToHost, st));
        VQ_HIP(hipStreamSynchronize(st));
    }
    if (idx.sharded()) idx.sum_over_shards(counts);
    size_t k = 0;
    for (auto& kv : table) {
        const size_t n = kv.second.anchors ? 2 * kv.second.anchors->size() : 0;
        kv.second.counts.assign(counts.begin() + k, counts.begin() + k + n);
        k += n;
    }
}

// K2 for wide leaves (union_dense.hip): a u32 key per doc of the shard's range in a slab, raised by one atomic max per posting, then compacted
// into k_union<write>'s output format.  The jobs run in groups whose slabs fit the budget; nothing comes back to the host between the
// launches, the lengths and largest values of all jobs are fetched in one read-back at the end.  A job's output slice is sized by its upper
// bound, min(postings, docs of the range).
namespace {
size_t union_dense_min() {  // jobs with more lists than this take the dense route
    static const size_t v = [] {
        const char* e = std::getenv("VQ_UNION_DENSE_MIN");
        return size_t(std::min<long long>(std::max<long long>(e ? std::atoll(e) : 64 * 64, 1), 64 * 64));  // (two levels of k_union take no more than 64 x 64)
    }();
    return v;
}
uint64_t union_dense_slab_budget() {  // bytes of slabs alive at once (a job always gets one)
    static const uint64_t v = [] {
        const char* e = std::getenv("VQ_UNION_DENSE_SLAB_MB");
        return uint64_t(std::min<long long>(std::max<long long>(e ? std::atoll(e) : 1024, 0), 1ll << 20)) << 20;
    }();
    return v;
}

void run_union_dense(const Index& idx, Workspace& ws, const std::vector<UnionJob*>& jobs, hipStream_t st) {
    if (jobs.empty()) return;
    const uint32_t range = idx.doc_hi - idx.doc_lo;
    const uint32_t job_blocks = std::max<uint32_t>(uint32_t((uint64_t(range) + kDenseBlockDocs - 1) / kDenseBlockDocs), 1u);
    const uint64_t slab_words = uint64_t(job_blocks) * kDenseBlockDocs;
    const size_t per_group = size_t(std::min<uint64_t>(std::max<uint64_t>(union_dense_slab_budget() / (slab_words * 4), 1), jobs.size()));
    struct Group {
        size_t job_begin, n_jobs, list_begin, n_lists;
        uint64_t postings;
    };
    std::vector<Group> groups;
    std::vector<UDenseList> lists;
    std::vector<UDenseJob> djobs(jobs.size());
    std::vector<uint64_t> cap(jobs.size());
    uint64_t out_cursor = 0;
    for (size_t jb = 0; jb < jobs.size(); jb += per_group) {
        Group g{jb, std::min(per_group, jobs.size() - jb), lists.size(), 0, 0};
        for (size_t k = 0; k < g.n_jobs; ++k) {
            UDenseJob& d = djobs[jb + k];
            d.slab_off = k * slab_words;
            d.out_off = out_cursor;
            d.block_begin = uint32_t(k) * job_blocks;
            d.n_blocks = job_blocks;
            d.result = uint32_t(jb + k);
            d.pad = 0;
            const uint64_t before = g.postings;
            for (auto& t : jobs[jb + k]->terms) {
                const PostingStore& ps = *t.store;
                if (!ps.len[t.token]) continue;  // (a shard without postings of the term)
                UDenseList u{};
                u.docs = ps.docs.as<uint32_t>() + ps.start[t.token];
                u.scores = ps.scores.as<uint16_t>() + ps.start[t.token];
                u.first = g.postings;
                u.term_score = t.score;
                u.job = uint32_t(k);
                lists.push_back(u);
                g.postings += ps.len[t.token];
            }
            cap[jb + k] = std::min<uint64_t>(g.postings - before, range);
            out_cursor += (cap[jb + k] + 8 + 3) / 4 * 4;  // 8 sentinel entries behind every list, starts stay 16-byte aligned
        }
        g.n_lists = lists.size() - g.list_begin;
        if (g.n_lists > 0xFFFFFFF0ull) throw VelociError(ERR_UNSUPPORTED, "leaf expansions of one batch with more than 2^32 posting lists");
        UDenseList end{};
        end.first = g.postings;
        lists.push_back(end);
        groups.push_back(g);
    }
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_jobs = al(lists.size() * sizeof(UDenseList)), o_res = o_jobs + al(djobs.size() * sizeof(UDenseJob)), o_cnt = o_res + al(jobs.size() * sizeof(UDenseResult)),
                 o_max = o_cnt + al(per_group * size_t(job_blocks) * 4), bytes = o_max + al(per_group * size_t(job_blocks) * 4);
    ws.d_union_dense_meta.ensure(bytes);
    ws.d_union_slab.ensure(per_group * slab_words * 4);
    ws.d_union_dense_docs.ensure(out_cursor * 4 + 64);
    ws.d_union_dense_vals.ensure(out_cursor * 4 + 64);
    uint8_t* m = ws.d_union_dense_meta.as<uint8_t>();
    const UDenseList* d_lists = reinterpret_cast<const UDenseList*>(m);
    const UDenseJob* d_jobs = reinterpret_cast<const UDenseJob*>(m + o_jobs);
    UDenseResult* d_res = reinterpret_cast<UDenseResult*>(m + o_res);
    uint32_t* d_cnt = reinterpret_cast<uint32_t*>(m + o_cnt);
    uint32_t* d_max = reinterpret_cast<uint32_t*>(m + o_max);
    uint32_t* slab = ws.d_union_slab.as<uint32_t>();
    VQ_HIP(hipMemcpyAsync(m, lists.data(), lists.size() * sizeof(UDenseList), hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemcpyAsync(m + o_jobs, djobs.data(), djobs.size() * sizeof(UDenseJob), hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemsetAsync(d_res, 0, jobs.size() * sizeof(UDenseResult), st));  // (a group without postings launches no scatter; its lists are empty all the same)
    const bool timed = idx.profile.enabled;
    std::vector<std::pair<size_t, size_t>> write_slots;  // (timed launch, group): the write pass's output bytes are known after the read-back
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const Group& g = groups[gi];
        const uint32_t n_blocks = uint32_t(g.n_jobs) * job_blocks;
        const uint64_t slab_bytes = g.n_jobs * slab_words * 4;
        {  // slab clear + scatter: 4 B per doc written, 6 B per posting read, one 4-byte atomic per posting
            LaunchTimer timer(timed, ws, st, K_UNION_DENSE_SCATTER, slab_bytes + g.postings * 10, g.postings * 6, g.n_jobs);
            VQ_HIP(hipMemsetAsync(slab, 0, slab_bytes, st));
            launch_union_dense_scatter(st, d_lists + g.list_begin, uint32_t(g.n_lists), g.postings, d_jobs + g.job_begin, slab, idx.doc_lo, range);
            VQ_HIP(hipGetLastError());
        }
        {  // 4 B per doc read; a count and a largest key per block written, read again by the prefix sums, the offsets written
            LaunchTimer timer(timed, ws, st, K_UNION_DENSE_COUNT, slab_bytes + uint64_t(n_blocks) * 20, slab_bytes, g.n_jobs);
            launch_union_dense_count(st, d_jobs + g.job_begin, uint32_t(g.n_jobs), n_blocks, slab, d_cnt, d_max, d_res);
            VQ_HIP(hipGetLastError());
        }
        {  // 4 B per doc read, 8 B per entry written (added below)
            LaunchTimer timer(timed, ws, st, K_UNION_DENSE_WRITE, slab_bytes + uint64_t(n_blocks) * 4, slab_bytes, g.n_jobs);
            if (timer.ws) write_slots.push_back({timer.slot, gi});
            launch_union_dense_write(st, d_jobs + g.job_begin, uint32_t(g.n_jobs), n_blocks, slab, d_cnt, idx.doc_lo, ws.d_union_dense_docs.as<uint32_t>(),
                                     ws.d_union_dense_vals.as<float>());
            VQ_HIP(hipGetLastError());
        }
    }
    std::vector<UDenseResult> res(jobs.size());
    VQ_HIP(hipMemcpyAsync(res.data(), d_res, res.size() * sizeof(UDenseResult), hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    for (size_t j = 0; j < jobs.size(); ++j) {
        if (res[j].len > cap[j]) throw VelociError(ERR_DEVICE, "dense union wrote more entries than its postings (internal)");
        if (res[j].len > 0xFFFFFFF0u) throw VelociError(ERR_UNSUPPORTED, "materialised leaf longer than 2^32 entries");
        UnionJob& job = *jobs[j];
        job.d_docs = ws.d_union_dense_docs.as<uint32_t>() + djobs[j].out_off;
        job.d_vals = ws.d_union_dense_vals.as<float>() + djobs[j].out_off;
        job.len = res[j].len;
        job.max_value = 0.0f;
        if (res[j].max_key) {
            const uint32_t bits = unorder_f32(res[j].max_key);
            std::memcpy(&job.max_value, &bits, 4);
        }
    }
    for (auto& [slot, gi] : write_slots) {
        uint64_t entries = 0;
        for (size_t k = 0; k < groups[gi].n_jobs; ++k) entries += res[groups[gi].job_begin + k].len + 8;
        ws.timed[slot].layout_bytes += entries * 8;
        ws.timed[slot].algorithmic_bytes += entries * 8;
    }
}
}  // namespace

void run_union_jobs(const Index& idx, Workspace& ws, UnionTable& table, hipStream_t st, int64_t dense_min) {
    const size_t dense_above = dense_min < 0 ? union_dense_min() : std::min<size_t>(size_t(dense_min), 64 * 64);  // (two levels of k_union take no more than 64 x 64)
    std::vector<UnionTaskH> l1, l2;
    std::vector<UnionJob*> dense;
    for (auto& kv : table) {
        UnionJob& job = kv.second;
        if (job.terms.size() > dense_above) {  // (the lists that are non-empty in the unsharded index: every shard takes the same route)
            dense.push_back(&job);
            continue;
        }
        std::vector<UList> raw;
        for (auto& t : job.terms) {
            const PostingStore& ps = *t.store;
            UList u{};
            u.docs = ps.docs.as<uint32_t>() + ps.start[t.token];
            u.scores = ps.scores.as<uint16_t>() + ps.start[t.token];
            u.len = ps.len[t.token];
            u.term_score = t.score;
            raw.push_back(u);
        }
        if (raw.size() <= 64) {
            UnionTaskH t;
            t.lists = std::move(raw);
            t.job = &job;
            l1.push_back(std::move(t));
        } else {
            UnionTaskH top;
            top.job = &job;
            for (size_t b = 0; b < raw.size(); b += 64) {
                UnionTaskH t;
                t.lists.assign(raw.begin() + b, raw.begin() + std::min(raw.size(), b + 64));
                t.parent = l2.size();
                l1.push_back(std::move(t));
            }
            l2.push_back(std::move(top));
        }
    }
    run_union_dense(idx, ws, dense, st);
    run_union_level(idx.profile.enabled, ws, l1, ws.d_union_docs[0], ws.d_union_vals[0], ws.d_union_max, ws.d_union_meta, st);
    for (auto& t : l1) {
        const uint32_t* d = ws.d_union_docs[0].as<uint32_t>() + t.out_off;
        const float* v = ws.d_union_vals[0].as<float>() + t.out_off;
        if (t.job) {
            t.job->d_docs = d;
            t.job->d_vals = v;
            t.job->max_value = t.max_value;
            t.job->len = t.len;
        } else {
            UList u{};
            u.docs = d;
            u.scores = v;
            u.len = t.len;
            u.term_score = 1.0f;
            u.flags = 1u;
            l2[t.parent].lists.push_back(u);
        }
    }
    if (!l2.empty()) {
        run_union_level(idx.profile.enabled, ws, l2, ws.d_union_docs[1], ws.d_union_vals[1], ws.d_union_max, ws.d_union_meta, st);  // (level 1 has synchronised)
        for (auto& t : l2) {
            t.job->max_value = t.max_value;
            t.job->d_docs = ws.d_union_docs[1].as<uint32_t>() + t.out_off;
            t.job->d_vals = ws.d_union_vals[1].as<float>() + t.out_off;
            t.job->len = t.len;
        }
    }
}

// K7: text locality of fields whose text ids are not anchors, for every (request, field) job of the batch (see kernels.hip, k_loc_*).
void run_locality_jobs(const Index& idx, Workspace& ws, LocalityTable& table, hipStream_t st) {
    std::vector<LocalityJob*> jobs;
    for (auto& kv : table) jobs.push_back(&kv.second);
    if (jobs.empty()) return;
    // all jobs of one table next to each other: one gather launch per tokens_to_text_id table
    std::stable_sort(jobs.begin(), jobs.end(), [](const LocalityJob* a, const LocalityJob* b) { return a->t2t_path < b->t2t_path; });
    const size_t nj = jobs.size();
    std::vector<LocJob> dj(nj);
    std::vector<LocRow> rows;
    std::vector<std::pair<size_t, size_t>> table_rows;  // per run of jobs over one table: [first row, end row)
    uint64_t cursor = 0;
    for (size_t j = 0; j < nj; ++j) {
        const KVStore& t2t = idx.kv.at(jobs[j]->t2t_path);
        const KVStore& t2a = idx.kv.at(jobs[j]->t2a_path);
        if (j == 0 || jobs[j]->t2t_path != jobs[j - 1]->t2t_path) table_rows.push_back({rows.size(), rows.size()});
        LocJob& J = dj[j];
        std::memset(&J, 0, sizeof J);
        J.t2a_vals = t2a.values.as<uint32_t>();
        J.t2a_start = t2a.d_row_start.as<uint64_t>();
        J.t2a_len = t2a.d_row_len.as<uint32_t>();
        J.t2a_key_base = t2a.key_base;
        J.t2a_num_keys = t2a.num_keys;
        J.seg_begin = uint32_t(cursor);
        for (uint32_t id : jobs[j]->tokens) {
            if (id < t2t.key_base || id - t2t.key_base >= t2t.num_keys) continue;
            const uint32_t r = id - t2t.key_base;
            uint64_t src = t2t.host_off[r], left = t2t.host_off[r + 1] - t2t.host_off[r];
            while (left) {  // long rows in pieces: one workgroup copies one piece
                const uint32_t piece = uint32_t(std::min<uint64_t>(left, 65536));
                rows.push_back(LocRow{src, cursor, piece, 0u});
                src += piece;
                cursor += piece;
                left -= piece;
            }
        }
        if (cursor > 0xFFFFFFF0ull) throw VelociError(ERR_UNSUPPORTED, "text_locality: more than 2^32 token->text entries in one batch");
        J.seg_end = uint32_t(cursor);
        table_rows.back().second = rows.size();
    }
    const uint32_t E = uint32_t(cursor);
    for (auto* j : jobs) {
        j->d_docs = nullptr;
        j->d_vals = nullptr;
        j->len = 0;
    }
    if (!E) return;
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    // meta: [jobs][rows][seg_begin u32][seg_end u32][counters u32][pair_begin u32][pair_end u32][out_len u32]
    const size_t o_jobs = 0, o_rows = al(nj * sizeof(LocJob)), o_sb = o_rows + al(rows.size() * sizeof(LocRow)), o_se = o_sb + al(nj * 4), o_cnt = o_se + al(nj * 4),
                 o_pb = o_cnt + al(nj * 4), o_pe = o_pb + al(nj * 4), o_len = o_pe + al(nj * 4), meta_bytes = o_len + al(nj * 4);
    ws.d_loc_meta.ensure(meta_bytes);
    uint8_t* m = ws.d_loc_meta.as<uint8_t>();
    std::vector<uint32_t> sb(nj), se(nj);
    for (size_t j = 0; j < nj; ++j) {
        sb[j] = dj[j].seg_begin;
        se[j] = dj[j].seg_end;
    }
    ws.d_loc_a.ensure(size_t(E) * 4 + 16);
    ws.d_loc_b.ensure(size_t(E) * 4 + 16);
    LaunchTimer timer(idx.profile.enabled, ws, st, K_LOCALITY, size_t(E) * 16, size_t(E) * 4, nj);
    VQ_HIP(hipMemcpyAsync(m + o_jobs, dj.data(), nj * sizeof(LocJob), hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemcpyAsync(m + o_rows, rows.data(), rows.size() * sizeof(LocRow), hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemcpyAsync(m + o_sb, sb.data(), nj * 4, hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemcpyAsync(m + o_se, se.data(), nj * 4, hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemsetAsync(m + o_cnt, 0, nj * 4, st));
    {
        size_t tr = 0;
        for (size_t j = 0; j < nj; ++j)
            if (j == 0 || jobs[j]->t2t_path != jobs[j - 1]->t2t_path) {
                const KVStore& t2t = idx.kv.at(jobs[j]->t2t_path);
                const auto [r0, r1] = table_rows[tr++];
                launch_loc_gather(st, reinterpret_cast<const LocRow*>(m + o_rows) + r0, uint32_t(r1 - r0), t2t.d_text_vals.as<uint32_t>(), ws.d_loc_a.as<uint32_t>());
            }
    }
    VQ_HIP(hipGetLastError());
    auto sort32 = [&](const uint32_t* in, uint32_t* out, uint32_t n, const uint32_t* b, const uint32_t* e) {
        const size_t need = seg_sort_u32(nullptr, 0, in, out, n, uint32_t(nj), b, e, st);
        if (need == size_t(-1)) throw VelociError(ERR_DEVICE, "segmented radix sort failed (size query)");
        ws.d_loc_tmp.ensure(need + 256);
        if (seg_sort_u32(ws.d_loc_tmp.p, need, in, out, n, uint32_t(nj), b, e, st) == size_t(-1)) throw VelociError(ERR_DEVICE, "segmented radix sort failed");
    };
    sort32(ws.d_loc_a.as<uint32_t>(), ws.d_loc_b.as<uint32_t>(), E, reinterpret_cast<const uint32_t*>(m + o_sb), reinterpret_cast<const uint32_t*>(m + o_se));
    // count pass: (anchor, boost) pairs per job
    launch_loc_expand(st, false, reinterpret_cast<const LocJob*>(m + o_jobs), uint32_t(nj), ws.d_loc_b.as<uint32_t>(), E, reinterpret_cast<uint32_t*>(m + o_cnt), nullptr);
    VQ_HIP(hipGetLastError());
    std::vector<uint32_t> totals(nj);
    VQ_HIP(hipMemcpyAsync(totals.data(), m + o_cnt, nj * 4, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    uint64_t P = 0, out_cursor = 0;
    std::vector<uint32_t> pb(nj), pe(nj);
    for (size_t j = 0; j < nj; ++j) {
        dj[j].pair_begin = pb[j] = uint32_t(P);
        P += totals[j];
        if (P > 0xFFFFFFF0ull) throw VelociError(ERR_UNSUPPORTED, "text_locality: more than 2^32 (anchor, boost) pairs in one batch");
        dj[j].pair_end = pe[j] = uint32_t(P);
        dj[j].out_off = uint32_t(out_cursor);
        out_cursor += (uint64_t(totals[j]) + 8 + 3) / 4 * 4;  // 8 sentinel entries behind every list, starts stay 16-byte aligned
    }
    ws.d_loc_docs.ensure(out_cursor * 4 + 64);
    ws.d_loc_vals.ensure(out_cursor * 4 + 64);
    if (P) {
        ws.d_loc_pairs_a.ensure(P * 8 + 16);
        ws.d_loc_pairs_b.ensure(P * 8 + 16);
        VQ_HIP(hipMemcpyAsync(m + o_jobs, dj.data(), nj * sizeof(LocJob), hipMemcpyHostToDevice, st));
        VQ_HIP(hipMemcpyAsync(m + o_pb, pb.data(), nj * 4, hipMemcpyHostToDevice, st));
        VQ_HIP(hipMemcpyAsync(m + o_pe, pe.data(), nj * 4, hipMemcpyHostToDevice, st));
        VQ_HIP(hipMemsetAsync(m + o_cnt, 0, nj * 4, st));
        launch_loc_expand(st, true, reinterpret_cast<const LocJob*>(m + o_jobs), uint32_t(nj), ws.d_loc_b.as<uint32_t>(), E, reinterpret_cast<uint32_t*>(m + o_cnt),
                          ws.d_loc_pairs_a.as<unsigned long long>());
        VQ_HIP(hipGetLastError());
        const size_t need = seg_sort_u64(nullptr, 0, ws.d_loc_pairs_a.as<unsigned long long>(), ws.d_loc_pairs_b.as<unsigned long long>(), uint32_t(P), uint32_t(nj),
                                         reinterpret_cast<const uint32_t*>(m + o_pb), reinterpret_cast<const uint32_t*>(m + o_pe), st);
        if (need == size_t(-1)) throw VelociError(ERR_DEVICE, "segmented radix sort failed (size query)");
        ws.d_loc_tmp.ensure(need + 256);
        if (seg_sort_u64(ws.d_loc_tmp.p, need, ws.d_loc_pairs_a.as<unsigned long long>(), ws.d_loc_pairs_b.as<unsigned long long>(), uint32_t(P), uint32_t(nj),
                         reinterpret_cast<const uint32_t*>(m + o_pb), reinterpret_cast<const uint32_t*>(m + o_pe), st) == size_t(-1))
            throw VelociError(ERR_DEVICE, "segmented radix sort failed");
    } else VQ_HIP(hipMemcpyAsync(m + o_jobs, dj.data(), nj * sizeof(LocJob), hipMemcpyHostToDevice, st));
    launch_loc_compact(st, reinterpret_cast<const LocJob*>(m + o_jobs), uint32_t(nj), ws.d_loc_pairs_b.as<unsigned long long>(), ws.d_loc_docs.as<uint32_t>(),
                       ws.d_loc_vals.as<float>(), reinterpret_cast<uint32_t*>(m + o_len));
    VQ_HIP(hipGetLastError());
    std::vector<uint32_t> lens(nj);
    VQ_HIP(hipMemcpyAsync(lens.data(), m + o_len, nj * 4, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    for (size_t j = 0; j < nj; ++j) {
        jobs[j]->d_docs = ws.d_loc_docs.as<uint32_t>() + dj[j].out_off;
        jobs[j]->d_vals = ws.d_loc_vals.as<float>() + dj[j].out_off;
        jobs[j]->len = lens[j];
    }
}

// K10: the 1:n boost lists of a batch (boost.rs:432-468).  Host: one gather descriptor per text id (its value_id_to_parent row).  Device: gather
// the value ids, sort them per job (value-id order is the order the reference applies the boosts in), k_b1n_map.
void run_boost1n_jobs(const Index& idx, Workspace& ws, Boost1nTable& table, hipStream_t st) {
    const double t_begin = now_ms();
    std::vector<Boost1nJob*> jobs;
    for (auto& kv : table) jobs.push_back(&kv.second);
    if (jobs.empty()) return;
    std::stable_sort(jobs.begin(), jobs.end(), [](const Boost1nJob* a, const Boost1nJob* b) { return a->to_parent_path < b->to_parent_path; });
    const size_t nj = jobs.size();
    std::vector<B1nJob> dj(nj);
    std::vector<LocRow> rows;
    std::vector<std::pair<size_t, size_t>> table_rows;  // per run of jobs over one value_id_to_parent table: [first row, end row)
    uint64_t cursor = 0, out_cursor = 0;
    for (size_t j = 0; j < nj; ++j) {
        const KVStore& to_parent = idx.kv.at(jobs[j]->to_parent_path);
        const KVStore& to_anchor = idx.kv.at(jobs[j]->to_anchor_path);
        const BoostColumn& col = idx.boost.at(jobs[j]->boost_path);
        if (j == 0 || jobs[j]->to_parent_path != jobs[j - 1]->to_parent_path) table_rows.push_back({rows.size(), rows.size()});
        B1nJob& J = dj[j];
        std::memset(&J, 0, sizeof J);
        J.boost_present = col.has_present ? col.present.as<uint32_t>() : nullptr;
        J.boost_values = col.values.as<float>();
        J.boost_key_base = col.key_base;
        J.boost_num_keys = col.num_keys;
        J.to_anchor_off = to_anchor.d_csr_off.as<uint64_t>();
        J.to_anchor_vals = to_anchor.d_text_vals.as<uint32_t>();
        J.to_anchor_key_base = to_anchor.key_base;
        J.to_anchor_num_keys = to_anchor.num_keys;
        J.doc_lo = idx.doc_lo;
        J.doc_hi = idx.doc_hi;
        J.seg_begin = uint32_t(cursor);
        for (uint32_t id : jobs[j]->text_ids) {
            if (id < to_parent.key_base || id - to_parent.key_base >= to_parent.num_keys) continue;
            const uint32_t r = id - to_parent.key_base;
            uint64_t src = to_parent.host_off[r], left = to_parent.host_off[r + 1] - to_parent.host_off[r];
            while (left) {
                const uint32_t piece = uint32_t(std::min<uint64_t>(left, 65536));
                rows.push_back(LocRow{src, cursor, piece, 0u});
                src += piece;
                cursor += piece;
                left -= piece;
            }
        }
        if (cursor > 0xFFFFFFF0ull) throw VelociError(ERR_UNSUPPORTED, "1:n field boost: more than 2^32 value ids in one batch");
        J.seg_end = uint32_t(cursor);
        J.out_off = uint32_t(out_cursor);
        out_cursor += (uint64_t(J.seg_end - J.seg_begin) + 8 + 3) / 4 * 4;  // 8 sentinel entries behind every list, starts stay 16-byte aligned
        if (out_cursor > 0xFFFFFFF0ull) throw VelociError(ERR_UNSUPPORTED, "1:n field boost: more than 2^32 value ids in one batch");
        table_rows.back().second = rows.size();
    }
    const uint32_t E = uint32_t(cursor);
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_jobs = 0, o_rows = al(nj * sizeof(B1nJob)), o_sb = o_rows + al(rows.size() * sizeof(LocRow)), o_se = o_sb + al(nj * 4), o_res = o_se + al(nj * 4),
                 meta_bytes = o_res + al(nj * sizeof(B1nResult));
    ws.d_b1n_meta.ensure(meta_bytes);
    ws.d_b1n_a.ensure(size_t(E) * 4 + 16);
    ws.d_b1n_b.ensure(size_t(E) * 4 + 16);
    ws.d_b1n_docs.ensure(out_cursor * 4 + 64);
    ws.d_b1n_vals.ensure(out_cursor * 4 + 64);
    uint8_t* m = ws.d_b1n_meta.as<uint8_t>();
    std::vector<uint32_t> sb(nj), se(nj);
    for (size_t j = 0; j < nj; ++j) {
        sb[j] = dj[j].seg_begin;
        se[j] = dj[j].seg_end;
    }
    const double t_rows = now_ms();
    LaunchTimer timer(idx.profile.enabled, ws, st, K_BOOST1N, size_t(E) * 24, size_t(E) * 12, nj);
    VQ_HIP(hipMemcpyAsync(m + o_jobs, dj.data(), nj * sizeof(B1nJob), hipMemcpyHostToDevice, st));
    if (!rows.empty()) VQ_HIP(hipMemcpyAsync(m + o_rows, rows.data(), rows.size() * sizeof(LocRow), hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemcpyAsync(m + o_sb, sb.data(), nj * 4, hipMemcpyHostToDevice, st));
    VQ_HIP(hipMemcpyAsync(m + o_se, se.data(), nj * 4, hipMemcpyHostToDevice, st));
    if (E) {
        size_t tr = 0;
        for (size_t j = 0; j < nj; ++j)
            if (j == 0 || jobs[j]->to_parent_path != jobs[j - 1]->to_parent_path) {
                const KVStore& to_parent = idx.kv.at(jobs[j]->to_parent_path);
                const auto [r0, r1] = table_rows[tr++];
                launch_loc_gather(st, reinterpret_cast<const LocRow*>(m + o_rows) + r0, uint32_t(r1 - r0), to_parent.d_text_vals.as<uint32_t>(), ws.d_b1n_a.as<uint32_t>());
            }
        VQ_HIP(hipGetLastError());
        const size_t need = seg_sort_u32(nullptr, 0, ws.d_b1n_a.as<uint32_t>(), ws.d_b1n_b.as<uint32_t>(), E, uint32_t(nj), reinterpret_cast<const uint32_t*>(m + o_sb),
                                         reinterpret_cast<const uint32_t*>(m + o_se), st);
        if (need == size_t(-1)) throw VelociError(ERR_DEVICE, "segmented radix sort failed (size query)");
        ws.d_b1n_tmp.ensure(need + 256);
        if (seg_sort_u32(ws.d_b1n_tmp.p, need, ws.d_b1n_a.as<uint32_t>(), ws.d_b1n_b.as<uint32_t>(), E, uint32_t(nj), reinterpret_cast<const uint32_t*>(m + o_sb),
                         reinterpret_cast<const uint32_t*>(m + o_se), st) == size_t(-1))
            throw VelociError(ERR_DEVICE, "segmented radix sort failed");
    }
    double t_sorted = 0;
    if (timing_enabled()) {
        VQ_HIP(hipStreamSynchronize(st));
        t_sorted = now_ms();
    }
    launch_b1n_map(st, reinterpret_cast<const B1nJob*>(m + o_jobs), uint32_t(nj), ws.d_b1n_b.as<uint32_t>(), ws.d_b1n_docs.as<uint32_t>(), ws.d_b1n_vals.as<float>(),
                   reinterpret_cast<B1nResult*>(m + o_res));
    VQ_HIP(hipGetLastError());
    std::vector<B1nResult> res(nj);
    VQ_HIP(hipMemcpyAsync(res.data(), m + o_res, nj * sizeof(B1nResult), hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    for (size_t j = 0; j < nj; ++j) {
        jobs[j]->d_docs = ws.d_b1n_docs.as<uint32_t>() + dj[j].out_off;
        jobs[j]->d_vals = ws.d_b1n_vals.as<float>() + dj[j].out_off;
        jobs[j]->len = res[j].len;
        jobs[j]->total = res[j].total;
        jobs[j]->ascending = !(res[j].flags & 1u);
        jobs[j]->several = (res[j].flags & 2u) != 0;
        jobs[j]->done = true;
    }
    if (timing_enabled()) {
        uint32_t longest = 0, n_several = 0;
        for (size_t j = 0; j < nj; ++j) {
            longest = std::max(longest, dj[j].seg_end - dj[j].seg_begin);
            n_several += jobs[j]->several ? 1u : 0u;
        }
        std::fprintf(stderr, "[vq timing] 1:n boost lists (K10): %zu jobs, %u value ids (longest list %u, %u with several values per anchor), %zu gather rows; host rows %.3f ms, gather + sort %.3f ms, map %.3f ms\n",
                     nj, E, longest, n_several, rows.size(), t_rows - t_begin, t_sorted - t_rows, now_ms() - t_sorted);
    }
}

// Count pre-pass: launches k_tile_scan in count mode for queries whose AND operands' result sizes the compiler needs
// (set_op.rs:388-393,439) and returns them per query.  Presence only: no scores are read.
static void run_count_queries(const Index& idx, Workspace& ws, const std::vector<CompiledQuery*>& cqs, std::vector<QueryCounts>& out, hipStream_t st) {
    const size_t n = cqs.size();
    out.assign(n, QueryCounts{});
    if (!n) return;
    std::vector<uint32_t> blob_off(n + 1, 0), span_base(n + 1, 0), qmap(n), counts_off(n + 1, 0);
    size_t lds_bytes = 0, desc_cap = 0;
    uint32_t stack_depth = 1;
    for (size_t i = 0; i < n; ++i) {
        const CompiledQuery& cq = *cqs[i];
        size_t desc = 0;
        const size_t bytes = pack_blob(cq, idx, nullptr, nullptr, 0, 0, {}, {}, &desc);
        blob_off[i + 1] = uint32_t(blob_off[i] + align_up(bytes, 16));
        span_base[i + 1] = span_base[i] + cq.n_spans;
        counts_off[i + 1] = counts_off[i] + cq.n_counts;
        qmap[i] = uint32_t(i);
        desc_cap = std::max(desc_cap, desc);
        stack_depth = std::max(stack_depth, cq.stack_depth);
    }
    desc_cap = align_up(desc_cap, 16);
    uint32_t list_table = 2;
    for (size_t i = 0; i < n; ++i) list_table = std::max<uint32_t>(list_table, uint32_t(cqs[i]->lists.size()));
    list_table = (list_table + 1u) & ~1u;
    const uint32_t cand_cap = 256;  // the candidate area doubles as the counter array (<= 256 counters)
    for (size_t i = 0; i < n; ++i)
        lds_bytes = std::max(lds_bytes, tile_scan_lds_bytes(uint32_t(cqs[i]->lists.size()) + cqs[i]->n_temps, uint32_t(cqs[i]->lists.size()), cqs[i]->tile_words,
                                                            stack_depth, cand_cap, uint32_t(desc_cap), false, list_table));
    if (lds_bytes > 160 * 1024) throw VelociError(ERR_UNSUPPORTED, "LDS tile larger than 160 KiB");
    const size_t o_off = align_up(blob_off[n], 256), o_span = o_off + align_up((n + 1) * 4, 256), o_qmap = o_span + align_up((n + 1) * 4, 256),
                 o_cnt = o_qmap + align_up(n * 4, 256), total = o_cnt + align_up(size_t(counts_off[n]) * 8, 256);
    std::vector<uint8_t> host(total, 0);
    ws.d_union_meta.ensure(total);
    uint8_t* dev = ws.d_union_meta.as<uint8_t>();
    for (size_t i = 0; i < n; ++i) pack_blob(*cqs[i], idx, host.data() + blob_off[i], dev + blob_off[i], 0, counts_off[i], {}, {});
    std::memcpy(host.data() + o_off, blob_off.data(), (n + 1) * 4);
    std::memcpy(host.data() + o_span, span_base.data(), (n + 1) * 4);
    std::memcpy(host.data() + o_qmap, qmap.data(), n * 4);
    VQ_HIP(hipMemcpyAsync(dev, host.data(), total, hipMemcpyHostToDevice, st));
    {
        uint64_t id_bytes = 0;  // presence only: the doc ids of every list
        for (size_t i = 0; i < n; ++i) id_bytes += 4ull * cqs[i]->total_len;
        LaunchTimer timer(idx.profile.enabled, ws, st, K_COUNT_PREPASS, id_bytes, id_bytes, n);
        launch_tile_scan(st, span_base[n], lds_bytes, dev, reinterpret_cast<const uint32_t*>(dev + o_off), reinterpret_cast<const uint32_t*>(dev + o_span),
                         reinterpret_cast<const uint32_t*>(dev + o_qmap), uint32_t(n), stack_depth, cand_cap, uint32_t(desc_cap), nullptr,
                         reinterpret_cast<unsigned long long*>(dev + o_cnt), nullptr, false, list_table);
    }
    VQ_HIP(hipGetLastError());
    std::vector<uint64_t> cnt(counts_off[n]);
    VQ_HIP(hipMemcpyAsync(cnt.data(), dev + o_cnt, cnt.size() * 8, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; ++i) {
        const CompiledQuery& cq = *cqs[i];
        const uint64_t* c = cnt.data() + counts_off[i];
        out[i].has_filter = !cq.fops.empty();
        out[i].filter_count = c[cq.n_counts - 1];
        for (size_t k = 0; k < cq.count_nodes.size(); ++k) out[i].nodes[cq.count_nodes[k]] = {c[2 * k], c[2 * k + 1]};
    }
}

// blob and descriptor size of a compiled query (a dry run of pack_blob), kept with it: the serial part of a step does not walk every query three times
static void size_blob(CompiledQuery& cq, const Index& idx) {
    if (cq.status != 0) return;
    size_t d = 0;
    cq.blob_bytes = pack_blob(cq, idx, nullptr, nullptr, 0, 0, {}, {}, &d);
    cq.desc_bytes = d;
}

// ---- run_partial: the host side of a step, phase by phase (the functions follow in the order run_partial calls them)

// A workspace for the batch: any free one (slot < 0), or the one the caller named, which then stays pinned until the batch is finished
static void acquire_workspace(const Index& idx, PartialBatch& pb, int slot) {
    if (slot < 0) {
        // any workspace: the first free one from the round-robin position on, never one that a batch holds by name (the chunks of a sharded step
        // in flight: waiting for one of those on the thread that has to end the step would never return)
        const uint32_t start = idx.next_ws.fetch_add(1);
        int fallback = -1;
        for (uint32_t k = 0; k < uint32_t(kWorkspaces) && !pb.lock.owns_lock(); ++k) {
            Workspace& w = idx.ws[(start + k) % kWorkspaces];
            if (w.pinned.load(std::memory_order_acquire)) continue;
            if (fallback < 0) fallback = int((start + k) % kWorkspaces);
            std::unique_lock<std::mutex> l(w.mu, std::try_to_lock);
            if (l.owns_lock() && !w.pinned.load(std::memory_order_acquire)) {
                pb.ws = &w;
                pb.lock = std::move(l);
            }
        }
        if (!pb.lock.owns_lock()) {
            if (fallback < 0) throw vqreq::VelociError(vqreq::ERR_INVALID_ARGUMENT, "every workspace of the index is held by a sharded step in flight: end a step first");
            pb.ws = &idx.ws[fallback];  // held by another thread's batch: it will be handed on
            pb.lock = std::unique_lock<std::mutex>(pb.ws->mu);
        }
    } else {
        pb.ws = &idx.ws[slot % kWorkspaces];
        pb.lock = std::unique_lock<std::mutex>(pb.ws->mu, std::try_to_lock);
        if (!pb.lock.owns_lock()) {
            if (pb.ws->pinned.load(std::memory_order_acquire)) throw vqreq::VelociError(vqreq::ERR_INVALID_ARGUMENT, "the workspace named for this batch is held by a step in flight");
            pb.lock = std::unique_lock<std::mutex>(pb.ws->mu);
        }
        pb.ws->pinned.store(true, std::memory_order_release);
        pb.pinned_ws = true;
    }
}

// What the pre-passes of one batch have produced so far; compile_batch owns it and hands every compilation pass its view
struct BatchTables {
    FuzzyTable fuzzy;          // dictionary scans of the fuzzy / prefix / regex leaves
    UnionTable unions;         // K2
    RangeTable ranges;
    LocalityTable localities;  // K7
    Boost1nTable boost1n;      // K10 (the compiler reaches it through boost_cache.device)
    Boost1nCache boost_cache;  // resolved 1:n boost lists, shared by the batch's requests and compilation passes
    // Pass 1 sees the dictionary scans and the 1:n cache and none of the job tables, whatever they hold: without a table a leaf ASKS for its job
    CompileInputs first_pass() {
        CompileInputs in;
        in.fuzzy = fuzzy.empty() ? nullptr : &fuzzy;
        in.boost_cache = &boost_cache;
        return in;
    }
    // Every later pass sees all of them, an empty table as null; the final pass also the count pre-pass's numbers for its query
    CompileInputs later_pass(const QueryCounts* counts = nullptr) {
        CompileInputs in = first_pass();
        in.unions = unions.empty() ? nullptr : &unions;
        in.ranges = ranges.empty() ? nullptr : &ranges;
        in.localities = localities.empty() ? nullptr : &localities;
        in.counts = counts;
        return in;
    }
};
struct CompileReport {  // what report_timing quotes of compile_batch
    double t_probes = 0, t_pass1 = 0, t_unions = 0, t_ranges = 0, t_compiled = 0;
    size_t probes = 0, unions = 0, ranges = 0;
};

// Pass 1: every request compiled once, from 64 requests on over the index's host threads.  Leaves `order`, the order the requests were taken in,
// and returns whether that was heaviest first.
static bool compile_first_pass(const Index& idx, PartialBatch& pb, const vqreq::Request* const* reqs, size_t n, BatchTables& tables, std::vector<uint32_t>& order) {
    // Requests are compiled heaviest first: a request's cost follows the terms its prefix / fuzzy leaves matched (their posting lists, the 1:n boost
    // lists behind them), which the dictionary scans have just counted; one such request can take as long as a hundred others, and claimed last
    // it alone would be the end of the parallel pass.
    const FuzzyTable& fuzzy = tables.fuzzy;
    order.resize(n);
    for (size_t i = 0; i < n; ++i) order[i] = uint32_t(i);
    const bool heavy_first = n >= 64 && !fuzzy.empty() && host_threads() > 1;
    if (heavy_first) {
        std::vector<uint64_t> weight(n, 0);
        std::function<void(const vqreq::SearchRequest&, uint64_t&)> walk = [&](const vqreq::SearchRequest& r, uint64_t& w) {
            if (r.kind == vqreq::SearchRequest::Search) {
                if (!needs_dictionary_scan(r.part)) return;
                auto it = fuzzy.find(fuzzy_key(r.part));
                if (it != fuzzy.end()) w += it->second.matches.size();
            } else
                for (auto& q : r.tree.queries) walk(q, w);
        };
        for (size_t i = 0; i < n; ++i)
            if (reqs[i] && reqs[i]->search_req) walk(*reqs[i]->search_req, weight[i]);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return weight[x] > weight[y]; });
    }
    const CompileInputs in = tables.first_pass();
    auto compile_range = [&](size_t b, size_t e) {
        for (size_t k = b; k < e; ++k) {
            const size_t i = order[k];
            if (!reqs[i]) {
                pb.queries[i].status = ERR_INVALID_ARGUMENT;
                pb.queries[i].error = "null request";
            } else {
                pb.queries[i] = compile_query(idx, *reqs[i], in);
                size_blob(pb.queries[i], idx);
            }
        }
    };
    if (n >= 64) {  // query compilation is independent per request: fan out over the index's host threads
        // Parts are claimed dynamically and shrink as the work runs out (guided scheduling: a part is 1/(2 x threads) of what is left, down to
        // one request): few claims while everybody is busy, single requests at the end — a worker that wakes late (an idle core takes ~0.1 ms,
        // a third of the whole job) still finds work, and requests of very different cost (a prefix leaf with a 1:n boost list takes 1000x a
        // plain AND) balance out.
        const std::vector<std::pair<size_t, size_t>> parts = guided_ranges(n, host_threads(), heavy_first ? 4 * host_threads() : 0);
        host_pool(idx).run(parts.size(), [&](size_t p) { compile_range(parts[p].first, parts[p].second); });
    } else compile_range(0, n);
    return heavy_first;
}

// Leaves that asked to be materialised first (K2): the union, locality and 1:n-boost jobs run once per batch, then the requests that asked are
// compiled again with the results — up to twice, around the range jobs
static void compile_with_jobs(const Index& idx, Workspace& ws, PartialBatch& pb, const vqreq::Request* const* reqs, const std::vector<uint32_t>& order, bool heavy_first,
                              BatchTables& tables, hipStream_t pst, CompileReport& rep) {
    std::vector<size_t> again;
    for (size_t k = 0; k < order.size(); ++k)
        if (const size_t i = order[k]; pb.queries[i].status == kStatusNeedsUnion || pb.queries[i].status == kStatusNeedsRanges) {
            again.push_back(i);
            for (auto& j : pb.queries[i].union_requests) tables.unions.emplace(j.key, j);
            for (auto& j : pb.queries[i].locality_requests) tables.localities.emplace(j.key, j);
            for (auto& j : pb.queries[i].boost1n_requests) tables.boost1n.emplace(j.key, j);
        }
    if (again.empty()) return;
    if (!tables.unions.empty()) {
        run_union_jobs(idx, ws, tables.unions, pst);
        // merged lengths over all shards (the AND summation order follows them)
        std::vector<uint64_t> lens;
        for (auto& kv : tables.unions) lens.push_back(kv.second.len);
        if (idx.can_sum_over_shards()) idx.sum_over_shards(lens);
        size_t k = 0;
        for (auto& kv : tables.unions) kv.second.global_len = lens[k++];
    }
    if (!tables.localities.empty()) run_locality_jobs(idx, ws, tables.localities, pst);
    if (!tables.boost1n.empty()) {
        run_boost1n_jobs(idx, ws, tables.boost1n, pst);
        tables.boost_cache.device = &tables.boost1n;
    }
    rep.t_unions = rep.t_ranges = now_ms();
    // Compile again with the jobs' results.  A 1:n boost list only shows once it is resolved (K10) whether an anchor carries several values:
    // those leaves then ask for a range pre-pass — which of the values apply follows the leaf's hits around each anchor (k_range_hits, on the
    // merged list of a materialised leaf) — and are compiled a third time.
    for (int round = 0; round < 2 && !again.empty(); ++round) {
        bool any_ranges = false;
        for (size_t i : again)
            if (pb.queries[i].status == kStatusNeedsRanges) {
                any_ranges = true;
                for (auto& j : pb.queries[i].range_requests) tables.ranges.emplace(j.key, j);
            }
        const bool ranges_ok = !any_ranges || !idx.sharded() || idx.can_sum_over_shards();
        if (any_ranges && ranges_ok) run_range_jobs(idx, ws, tables.ranges, tables.unions, pst);
        rep.t_ranges = now_ms();
        const CompileInputs in = tables.later_pass();
        auto recompile = [&](size_t b, size_t e) {
            for (size_t k = b; k < e; ++k) {
                CompiledQuery& q = pb.queries[again[k]];
                if (q.status == kStatusNeedsRanges && !ranges_ok) {
                    q.status = ERR_UNSUPPORTED;
                    q.error = "unsupported on the MI355X query path: 1:n field boost with several boosted values on one anchor, on a sharded index without vq_index_set_allreduce";
                    continue;
                }
                q = compile_query(idx, *reqs[again[k]], in);
                if (q.status == kStatusNeedsUnion || (q.status == kStatusNeedsRanges && round == 1)) {
                    q.status = ERR_UNSUPPORTED;
                    q.error = "unsupported on the MI355X query path: leaf expansion changed between compilation passes (internal)";
                }
                size_blob(q, idx);
            }
        };
        if (again.size() >= 8 && host_threads() > 1) {
            const std::vector<std::pair<size_t, size_t>> parts = guided_ranges(again.size(), host_threads(), heavy_first ? 4 * host_threads() : 0);
            host_pool(idx).run(parts.size(), [&](size_t p) { recompile(parts[p].first, parts[p].second); });
        } else recompile(0, again.size());
        std::vector<size_t> still;
        for (size_t i : again)
            if (pb.queries[i].status == kStatusNeedsRanges) still.push_back(i);
        again.swap(still);
    }
}

// ANDs whose summation order / label follow run-time operand sizes: count pre-pass, then the final compilation
static void compile_with_counts(const Index& idx, Workspace& ws, PartialBatch& pb, const vqreq::Request* const* reqs, BatchTables& tables, hipStream_t pst) {
    std::vector<size_t> need;
    std::vector<CompiledQuery*> cqs;
    for (size_t i = 0; i < pb.queries.size(); ++i)
        if (pb.queries[i].status == kStatusNeedsCounts) {
            need.push_back(i);
            cqs.push_back(&pb.queries[i]);
        }
    if (need.empty()) return;
    std::vector<QueryCounts> counts;
    run_count_queries(idx, ws, cqs, counts, pst);
    if (idx.sharded()) {  // result sizes are sums over the shards
        auto each = [&](auto&& f) {  // every number of the counts, in one order
            for (auto& c : counts) {
                f(c.filter_count);
                for (auto& kv : c.nodes) f(kv.second.first), f(kv.second.second);
            }
        };
        std::vector<uint64_t> flat;
        each([&](uint64_t& v) { flat.push_back(v); });
        idx.sum_over_shards(flat);
        size_t k = 0;
        each([&](uint64_t& v) { v = flat[k++]; });
    }
    for (size_t k = 0; k < need.size(); ++k) {
        CompiledQuery& q = pb.queries[need[k]];
        q = compile_query(idx, *reqs[need[k]], tables.later_pass(&counts[k]));
        if (q.status < 0) {
            q.status = ERR_UNSUPPORTED;
            q.error = "unsupported on the MI355X query path: query still needs a pre-pass after the count pre-pass (internal)";
        }
    }
}

// Dictionary scans (fuzzy / prefix leaves) of the whole batch, then its compilation passes with the pre-passes between them: pb.queries
static CompileReport compile_batch(const Index& idx, Workspace& ws, PartialBatch& pb, const vqreq::Request* const* reqs, size_t n, hipStream_t st) {
    CompileReport rep;
    BatchTables tables;
    for (size_t i = 0; i < n; ++i)
        if (reqs[i]) collect_fuzzy_probes(idx, *reqs[i], tables.fuzzy);
    static const bool pre_own = std::getenv("VQ_PRE_ON_SCAN_STREAM") == nullptr;
    hipStream_t pst = pre_own && idx.pre_stream ? idx.pre_stream : st;  // the pre-passes' stream (see Index::pre_stream)
    if (!tables.fuzzy.empty()) run_fuzzy_probes(idx, ws, tables.fuzzy, pst);
    rep.t_probes = now_ms();
    pb.queries.reserve(n);
    pb.slot.assign(n, UINT32_MAX);
    pb.queries.resize(n);
    std::vector<uint32_t> order;
    const bool heavy_first = compile_first_pass(idx, pb, reqs, n, tables, order);
    rep.t_pass1 = rep.t_unions = rep.t_ranges = now_ms();
    if (timing_enabled() && std::getenv("VQ_TIMING_SUB")) {  // (tools/host_profile.py stops at the first launch: the running totals, pass 1 only)
        std::fprintf(stderr, "[vq timing] pass 1 of %zu: %.3f ms wall;", n, rep.t_pass1 - rep.t_probes);
        for (int k = 0; k < 10; ++k) std::fprintf(stderr, " [%d] %.3f", k, g_compile_ns[k].load() * 1e-6);
        std::fprintf(stderr, "\n");
    }
    compile_with_jobs(idx, ws, pb, reqs, order, heavy_first, tables, pst, rep);
    compile_with_counts(idx, ws, pb, reqs, tables, pst);
    rep.t_compiled = now_ms();
    rep.probes = tables.fuzzy.size(), rep.unions = tables.unions.size(), rep.ranges = tables.ranges.size();
    return rep;
}

// Spans per query: a small batch is split further, and requests of very different weight get spans in proportion to their postings
static void size_spans(std::vector<CompiledQuery>& queries) {
    const size_t n = queries.size();
    // a small batch (one query = the latency case) would leave most of the chip idle with spans sized for streaming efficiency:
    // split its queries further until the launch holds about one wave per SIMD of every CU
    static const uint64_t target1 = [] {
        const char* e = std::getenv("VQ_SPAN_TARGET");
        return uint64_t(e ? std::atoll(e) : 2048);
    }();
    // (one request: 2048 spans — its merge is serial in the span count; more requests merge in parallel: up to one wave per slot)
    const uint64_t target = std::min<uint64_t>(target1 + 64 * uint64_t(n - 1), std::max<uint64_t>(target1, 5120));
    uint64_t have = 0, total_postings = 0;
    for (const CompiledQuery& cq : queries)
        if (cq.status == 0) have += cq.n_spans, total_postings += cq.total_len;
    if (have && have * 3 <= target * 2) {
        const uint64_t f = (target + have - 1) / have;
        for (CompiledQuery& cq : queries)
            if (cq.status == 0) cq.n_spans = uint32_t(std::max<uint64_t>(cq.n_spans, std::min<uint64_t>(uint64_t(cq.n_spans) * f, cq.max_spans)));
    }
    // Requests of very different weight in one launch (a prefix leaf over a third of the documents beside exact matches of a few): the launch
    // ends with the longest span, so a request gets spans in proportion to its postings — as many as keep every span of the launch near
    // total / target postings, but no span below 4096 (bench_jmdict shape, 256 requests: k_tile_scan 4.1 -> 0.8 ms)
    static const bool weighted = std::getenv("VQ_NO_WEIGHTED_SPANS") == nullptr;
    if (weighted && n > 1 && total_postings) {
        const uint64_t per_span = std::max<uint64_t>(total_postings / target, 4096);
        for (CompiledQuery& cq : queries) {
            if (cq.status != 0) continue;
            const uint64_t want = std::min<uint64_t>((cq.total_len + per_span - 1) / per_span, cq.max_spans);
            cq.n_spans = uint32_t(std::max<uint64_t>(cq.n_spans, want));
        }
    }
}

// Where the batch's device queries lie, per slot: span keys, part of the partial, facet histograms and outputs; the totals the launches are sized by
struct BatchLayout {
    uint32_t nq = 0;
    uint64_t total_keys = 0, total_hist = 0, total_span_keys = 0, total_spans = 0, blob_bytes = 0;
    uint32_t max_lists = 1, stack_depth = 1;
    std::vector<uint32_t> keys_base, part_keys_off;
    std::vector<std::vector<uint32_t>> hist_offs, fac_out_offs;
};
// Slots of the queries that compiled, their offsets, the facet jobs, pb.layout
static BatchLayout plan_layout(const Index& idx, PartialBatch& pb) {
    BatchLayout L;
    std::vector<FacetJob> jobs;
    uint32_t fac_out_total = 0;
    for (size_t i = 0; i < pb.queries.size(); ++i) {
        CompiledQuery& cq = pb.queries[i];
        if (cq.status != 0) continue;
        pb.slot[i] = L.nq++;
        L.keys_base.push_back(uint32_t(L.total_span_keys));
        L.part_keys_off.push_back(uint32_t(L.total_keys));
        L.total_span_keys += uint64_t(cq.n_spans) * cq.top_k;
        L.total_keys += cq.top_k;
        L.total_spans += cq.n_spans;
        std::vector<uint32_t> ho, fo;
        for (auto& f : cq.facets) {
            ho.push_back(uint32_t(L.total_hist));
            fo.push_back(fac_out_total);
            jobs.push_back(FacetJob{uint32_t(L.total_hist), f.num_values, f.top, fac_out_total});
            L.total_hist += f.num_values;
            fac_out_total += f.top;
        }
        L.hist_offs.push_back(std::move(ho));
        L.fac_out_offs.push_back(std::move(fo));
        if (!cq.blob_bytes) size_blob(cq, idx);  // (normally taken on the compiling thread)
        L.blob_bytes += cq.blob_bytes;
        L.max_lists = std::max<uint32_t>(L.max_lists, uint32_t(cq.lists.size()));
        L.stack_depth = std::max(L.stack_depth, cq.stack_depth);
    }
    if (L.total_span_keys > 0xFFFFFFFFull || L.total_hist > 0xFFFFFFFFull || L.total_spans > 0x7FFFFFFFull)
        throw VelociError(ERR_UNSUPPORTED, "batch too large for 32-bit workspace offsets: split the batch");
    pb.nq_dev = L.nq;
    pb.total_spans = uint32_t(L.total_spans);
    pb.n_facet_jobs = uint32_t(jobs.size());
    pb.total_facet_out = fac_out_total;
    pb.facet_jobs = std::move(jobs);

    PartialLayout& lay = pb.layout;
    lay.nq = L.nq;
    lay.total_keys = L.total_keys;
    lay.total_hist = L.total_hist;
    lay.off_hits = 0;
    lay.off_stats = align_up(size_t(L.nq) * 8, 16);
    lay.off_keys = lay.off_stats + align_up(size_t(L.nq) * 8, 16);
    lay.off_hist = align_up(lay.off_keys + size_t(L.total_keys) * 8, 256);  // == bytes of the all-gathered part
    lay.bytes = align_up(lay.off_hist + size_t(L.total_hist) * 4, 256);
    return L;
}

// One (span_base, qmap) table per scan launch, in launch order: span_base = prefix sums of n_spans over the launch's queries (and a closing
// entry), qmap = the blob slot of its k-th query.  The tables lie one behind the other, each as long as its launch has queries.
enum : uint32_t { T_LEAF_F32 = 0, T_RICH, T_PROBE, T_AND = T_PROBE + kProbeShapes, T_SIMPLE, T_UNION, T_WIDE, T_TILE, kScanTables };
struct ScanTable {
    uint32_t *span_base = nullptr, *qmap = nullptr;             // host side of the upload area
    const uint32_t *d_span_base = nullptr, *d_qmap = nullptr;  // ... and where the launch finds them
    uint32_t n = 0, spans = 0;                       // queries, spans
};
static uint32_t table_of(const CompiledQuery& cq) {
    switch (cq.kclass) {
        case K_SCAN_LEAF_F32: return T_LEAF_F32;
        case K_SCAN_RICH: return T_RICH;
        case K_SCAN_PROBE: {  // a kernel per shape: OR / AND of ND operands beside the cover, from ND = 2 on per number of array operands
            if (sf_probe_or(cq.simple_flags)) return T_PROBE + kProbeOr;
            const uint32_t nd = cq.simple_n - 1, na = uint32_t(__builtin_popcount(sf_array_mask(cq.simple_flags)));
            return T_PROBE + (nd <= 1 ? kProbeAnd1 : nd == 2 ? kProbeAnd2A0 + na : kProbeAnd3A0 + na);
        }
        case K_SCAN_AND: return T_AND;
        case K_SCAN_SIMPLE: return T_SIMPLE;
        case K_SCAN_UNION: return T_UNION;
        case K_SCAN_WIDE: return T_WIDE;
        case K_TILE_SCAN: return T_TILE;
        default: throw VelociError(ERR_DEVICE, "query without a scan class (internal)");
    }
}
// The scan tables inside the upload area [blobs][blob_off][span tables][qmap tables][facet jobs] and each class's launch parameters
struct ScanPlan {
    ScanTable tabs[kScanTables];
    size_t up_bytes = 0;  // of the upload area
    bool union_has_or = false, facets_rich = false;
    uint32_t scatter_and = 0, scatter_simple = 0, scatter_rich = 0;  // id (scattered) lists per query: they alone need an LDS tile in k_scan_simple
    uint32_t leaves_wide = 0, scatter_wide = 0;
    struct ProbeParams {
        uint32_t na_seen = 0, arr_slot = 0;  // bit NA: a query with NA array operands; words of an array operand's LDS slot (the fullest tile of the shape's array lists)
    } probe[kProbeShapes];
    bool any_probe = false;
    uint64_t cls_layout[K_COUNT_] = {}, cls_algo[K_COUNT_] = {}, cls_q[K_COUNT_] = {};
};
// Packs the blobs and fills the scan tables in the workspace's pinned upload buffer; sets the batch's device addresses inside the upload area
static ScanPlan pack_upload(const Index& idx, PartialBatch& pb, const BatchLayout& L) {
    ScanPlan P;
    Workspace& ws = *pb.ws;
    const PartialLayout& lay = pb.layout;
    const uint32_t nq = L.nq;
    const size_t up_blob_off = align_up(L.blob_bytes, 256);
    const size_t tbl = align_up(size_t(nq + kScanTables) * 4, 256);
    const size_t up_span = up_blob_off + align_up(size_t(nq + 1) * 4, 256);
    const size_t up_qmap = up_span + tbl;
    const size_t up_jobs = up_qmap + tbl;
    P.up_bytes = up_jobs + align_up(pb.facet_jobs.size() * sizeof(FacetJob), 256) + 256;
    ws.h_up.ensure(P.up_bytes);
    ws.d_up.ensure(P.up_bytes);
    uint8_t* hup = ws.h_up.as<uint8_t>();
    uint8_t* dup = ws.d_up.as<uint8_t>();
    size_t off = 0;
    uint32_t* hbo = reinterpret_cast<uint32_t*>(hup + up_blob_off);
    uint32_t qi = 0;
    for (const CompiledQuery& cq : pb.queries) {
        if (cq.status != 0) continue;
        hbo[qi] = uint32_t(off);
        const size_t packed = pack_blob(cq, idx, hup + off, dup + off, L.keys_base[qi], L.part_keys_off[qi], L.hist_offs[qi], L.fac_out_offs[qi], nullptr,
                                        pb.profiled ? uint32_t((lay.off_stats - lay.off_hits) / 8 + qi) : 0u);  // 0: the kernels count nothing
        if (packed != cq.blob_bytes) throw VelociError(ERR_DEVICE, "query blob changed size between compilation and packing (internal)");
        off += packed;
        ++qi;
        ++P.tabs[table_of(cq)].n;  // pass 1: how many queries every table holds
    }
    hbo[nq] = uint32_t(off);
    uint32_t at = 0;
    for (ScanTable& t : P.tabs) {  // ... which places them
        t.span_base = reinterpret_cast<uint32_t*>(hup + up_span) + at;
        t.qmap = reinterpret_cast<uint32_t*>(hup + up_qmap) + at;
        t.d_span_base = reinterpret_cast<const uint32_t*>(dup + up_span) + at;
        t.d_qmap = reinterpret_cast<const uint32_t*>(dup + up_qmap) + at;
        at += t.n + 1;
        t.n = 0;
    }
    qi = 0;
    for (const CompiledQuery& cq : pb.queries) {  // pass 2: the tables' entries and the launch parameters
        if (cq.status != 0) continue;
        const uint32_t ti = table_of(cq);
        ScanTable& t = P.tabs[ti];
        t.span_base[t.n] = t.spans;
        t.qmap[t.n++] = qi;
        t.spans += cq.n_spans;
        const uint32_t n_scatter = cq.simple_n - uint32_t(__builtin_popcount(sf_bitmap_mask(cq.simple_flags)));
        switch (cq.kclass) {
            case K_SCAN_WIDE:
                P.leaves_wide = std::max<uint32_t>(P.leaves_wide, cq.wide.n_leaves);
                P.scatter_wide = std::max<uint32_t>(P.scatter_wide, cq.wide.n_leaves - uint32_t(__builtin_popcount(cq.wide.bitmap_mask)));
                break;
            case K_SCAN_RICH:
                P.facets_rich = P.facets_rich || !cq.facets.empty();
                P.scatter_rich = std::max<uint32_t>(P.scatter_rich, n_scatter + cq.simple2.n_side);
                break;
            case K_SCAN_UNION: P.union_has_or = P.union_has_or || cq.simple_n > 1; break;
            case K_SCAN_PROBE: {
                ScanPlan::ProbeParams& pp = P.probe[ti - T_PROBE];
                pp.na_seen |= 1u << uint32_t(__builtin_popcount(sf_array_mask(cq.simple_flags)));
                pp.arr_slot = std::max(pp.arr_slot, cq.probe_arr_gran * 4u);
                P.any_probe = true;
                break;
            }
            case K_SCAN_AND: P.scatter_and = std::max(P.scatter_and, n_scatter); break;
            case K_SCAN_SIMPLE: P.scatter_simple = std::max(P.scatter_simple, n_scatter); break;
            default: break;
        }
        pb.qclass.push_back(uint8_t(cq.kclass));
        P.cls_layout[cq.kclass] += cq.layout_bytes;
        P.cls_algo[cq.kclass] += cq.algorithmic_bytes;
        P.cls_q[cq.kclass] += 1;
        ++qi;
    }
    for (ScanTable& t : P.tabs) t.span_base[t.n] = t.spans;
    if (!pb.facet_jobs.empty()) std::memcpy(hup + up_jobs, pb.facet_jobs.data(), pb.facet_jobs.size() * sizeof(FacetJob));
    pb.d_blobs = dup;
    pb.d_blob_off = reinterpret_cast<const uint32_t*>(dup + up_blob_off);
    pb.d_facet_jobs = reinterpret_cast<const FacetJob*>(dup + up_jobs);
    return P;
}

// Upload, the batch's partial, then one launch per scan table that holds spans, k_merge_spans behind them, and the event finish_batch waits for
static void launch_scans(const Index& idx, PartialBatch& pb, const BatchLayout& L, const ScanPlan& P, int64_t arena_offset) {
    Workspace& ws = *pb.ws;
    const PartialLayout& lay = pb.layout;
    hipStream_t st = idx.stream;
    VQ_HIP(hipMemcpyAsync(ws.d_up.as<uint8_t>(), ws.h_up.as<uint8_t>(), P.up_bytes, hipMemcpyHostToDevice, st));
    ws.d_span_keys.ensure(size_t(L.total_span_keys) * 8 + 16);
    if (arena_offset >= 0) {  // a chunk of a sharded step with one collective: its partial lives in the index's arena
        if (size_t(arena_offset) % 256 || size_t(arena_offset) + lay.bytes > Index::kArenaBytes)
            throw VelociError(ERR_UNSUPPORTED, "partial arena: the step's partials do not fit (" + std::to_string(size_t(arena_offset) + lay.bytes) + " bytes)");
        idx.arena.ensure(Index::kArenaBytes);
        pb.d_partial = idx.arena.as<uint8_t>() + arena_offset;
    } else {
        ws.d_partial.ensure(lay.bytes);
        pb.d_partial = ws.d_partial.as<uint8_t>();
    }
    VQ_HIP(hipMemsetAsync(pb.d_partial, 0, lay.bytes, st));

    // what the launches are sized by, over ALL device queries of the batch (k_tile_scan's descriptor and list-table room too, whoever it serves)
    uint32_t max_top_k = 1;
    uint32_t desc_cap = 0;  // bytes of the largest query descriptor (staged into LDS by every workgroup)
    bool facets_generic = false;  // k_tile_scan queries with facets: room for the LDS counter cache behind the descriptor
    static const bool no_facet_cache = std::getenv("VQ_NO_FACET_CACHE") != nullptr;
    for (const CompiledQuery& cq : pb.queries) {
        if (cq.status != 0) continue;
        max_top_k = std::max(max_top_k, cq.top_k);
        desc_cap = std::max(desc_cap, uint32_t(cq.desc_bytes));
        if (cq.kclass == K_TILE_SCAN && !cq.facets.empty()) facets_generic = !no_facet_cache;
    }
    desc_cap = uint32_t(align_up(desc_cap, 16));
    if (facets_generic) desc_cap += 2 * 1024 * 4;
    static const uint32_t cand_min = [] {
        const char* e = std::getenv("VQ_CAND_CAP");  // (a small buffer is pruned — and its threshold raised — sooner: 64 beats 256 by 2-7 %, 32 beats 64 by 1-2 %)
        return uint32_t(e ? std::max(32, std::atoi(e)) : 32);
    }();
    uint32_t cand_cap = cand_min;  // power of two >= 2 * top_k: candidate keys a workgroup keeps in LDS
    while (cand_cap < 2 * max_top_k) cand_cap <<= 1;
    const uint32_t list_table = (std::max<uint32_t>(L.max_lists, 2) + 1u) & ~1u;  // k_tile_scan sizes its per-list LDS arrays to the launch's longest list table
    static const bool tile_queue = std::getenv("VQ_NO_QUEUE") == nullptr;  // k_tile_scan: survivors of several tiles share a scoring round
    size_t lds_bytes = 0;
    for (const CompiledQuery& cq : pb.queries)
        if (cq.status == 0 && cq.kclass == K_TILE_SCAN)
            lds_bytes = std::max(lds_bytes, tile_scan_lds_bytes(uint32_t(cq.lists.size()) + cq.n_temps, uint32_t(cq.lists.size()), cq.tile_words, L.stack_depth, cand_cap, desc_cap,
                                                                tile_queue && !cq.simple_n, list_table));
    if (lds_bytes > 160 * 1024) throw VelociError(ERR_UNSUPPORTED, "LDS tile larger than 160 KiB");

    auto hits_ptr = reinterpret_cast<unsigned long long*>(pb.d_partial + lay.off_hits);
    auto hist_ptr = reinterpret_cast<uint32_t*>(pb.d_partial + lay.off_hist);
    auto keys_ptr = ws.d_span_keys.as<unsigned long long>();
    // one launch per table that holds spans, timed as its profile class, the launch error taken behind each
    auto scan = [&](uint32_t table, int k, auto&& launch) {
        if (const ScanTable& t = P.tabs[table]; t.spans) {
            LaunchTimer lt(pb.profiled, ws, st, k, P.cls_layout[k], P.cls_algo[k], P.cls_q[k]);
            launch(t);
        }
        VQ_HIP(hipGetLastError());
    };
    scan(T_LEAF_F32, K_SCAN_LEAF_F32, [&](const ScanTable& t) { launch_scan_leaf_f32(st, t.spans, pb.d_blobs, pb.d_blob_off, t.d_span_base, t.d_qmap, t.n, cand_cap, keys_ptr, hits_ptr, hist_ptr); });
    scan(T_RICH, K_SCAN_RICH, [&](const ScanTable& t) { launch_scan_simple(st, true, P.scatter_rich, t.spans, pb.d_blobs, pb.d_blob_off, t.d_span_base, t.d_qmap, t.n, cand_cap, keys_ptr, hits_ptr, hist_ptr, P.facets_rich); });
    if (P.any_probe) {  // (one timer over the shape kernels: the profile class is the sum of them)
        LaunchTimer lt(pb.profiled, ws, st, K_SCAN_PROBE, P.cls_layout[K_SCAN_PROBE], P.cls_algo[K_SCAN_PROBE], P.cls_q[K_SCAN_PROBE]);
        static const bool trace = std::getenv("VQ_PROBE_TRACE") != nullptr;  // tools: what every shape kernel of a launch was given
        for (uint32_t c = 0; c < kProbeShapes; ++c)
            if (const ScanTable& t = P.tabs[T_PROBE + c]; t.spans && trace)
                std::fprintf(stderr, "probe launch: shape %u, %u queries, %u spans, array slot %u words (fullest tile: %u granules), NA seen 0x%x\n", c, t.n, t.spans,
                             P.probe[c].arr_slot, P.probe[c].arr_slot / 4, P.probe[c].na_seen);
        for (uint32_t c = 0; c < kProbeShapes; ++c)
            if (const ScanTable& t = P.tabs[T_PROBE + c]; t.spans)
                launch_scan_probe_shape(st, c, P.probe[c].na_seen, P.probe[c].arr_slot, t.spans, pb.d_blobs, pb.d_blob_off, t.d_span_base, t.d_qmap, t.n, cand_cap, keys_ptr, hits_ptr);
    }
    VQ_HIP(hipGetLastError());
    scan(T_AND, K_SCAN_AND, [&](const ScanTable& t) { launch_scan_simple(st, false, P.scatter_and, t.spans, pb.d_blobs, pb.d_blob_off, t.d_span_base, t.d_qmap, t.n, cand_cap, keys_ptr, hits_ptr, hist_ptr); });
    // (16384-doc tiles pay off for ORs too once LDS no longer bounds the occupancy)
    scan(T_SIMPLE, K_SCAN_SIMPLE, [&](const ScanTable& t) { launch_scan_simple(st, false, P.scatter_simple, t.spans, pb.d_blobs, pb.d_blob_off, t.d_span_base, t.d_qmap, t.n, cand_cap, keys_ptr, hits_ptr, hist_ptr); });
    scan(T_UNION, K_SCAN_UNION, [&](const ScanTable& t) { launch_scan_union(st, P.union_has_or, t.spans, pb.d_blobs, pb.d_blob_off, t.d_span_base, t.d_qmap, t.n, cand_cap, keys_ptr, hits_ptr); });
    scan(T_WIDE, K_SCAN_WIDE, [&](const ScanTable& t) { launch_scan_wide(st, P.leaves_wide, P.scatter_wide, t.spans, pb.d_blobs, pb.d_blob_off, t.d_span_base, t.d_qmap, t.n, cand_cap, keys_ptr, hits_ptr); });
    scan(T_TILE, K_TILE_SCAN, [&](const ScanTable& t) { launch_tile_scan(st, t.spans, lds_bytes, pb.d_blobs, pb.d_blob_off, t.d_span_base, t.d_qmap, t.n, L.stack_depth, cand_cap, desc_cap, keys_ptr, hits_ptr, hist_ptr, tile_queue, list_table, facets_generic); });
    {
        LaunchTimer t(pb.profiled, ws, st, K_MERGE_SPANS, L.total_span_keys * 8 + L.total_keys * 8, L.total_span_keys * 8 + L.total_keys * 8, L.nq);
        launch_merge_spans(st, L.nq, pb.d_blobs, pb.d_blob_off, keys_ptr, reinterpret_cast<unsigned long long*>(pb.d_partial + lay.off_keys));
    }
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipEventRecord(ws.ev_done, st));
    pb.launched = true;
}

// VQ_TIMING: the step's host time by phase (tools/compile_scaling.sh cuts columns out of the "n=" line)
static void report_timing(size_t n, double t_start, const CompileReport& c, double t_layout, double t_packed, const ScanTable* tabs) {
    if (!timing_enabled()) return;
    std::fprintf(stderr, "[vq timing] n=%zu compile %.3f ms (dictionary scans %.3f [%zu probes], pass 1 %.3f, unions %.3f [%zu jobs], pass 2 %.3f), range jobs %.3f [%zu], spans generic/simple/and/rich/union %u/%u/%u/%u/%u, pack+launch %.3f ms\n", n,
                 c.t_compiled - t_start, c.t_probes - t_start, c.probes, c.t_pass1 - c.t_probes, c.t_unions - c.t_pass1, c.unions, c.t_compiled - c.t_ranges,
                 c.t_ranges - c.t_unions, c.ranges, tabs[T_TILE].spans, tabs[T_SIMPLE].spans, tabs[T_AND].spans, tabs[T_RICH].spans, tabs[T_UNION].spans + tabs[T_LEAF_F32].spans, now_ms() - c.t_compiled);
    std::fprintf(stderr, "[vq timing] pack+launch: span sizing + layout %.3f, blobs + tables %.3f, upload + launches %.3f ms\n", t_layout - c.t_compiled, t_packed - t_layout, now_ms() - t_packed);
    // thread-time inside compile_query since the last batch (all passes, all threads)
    uint64_t v[16];
    for (int k = 0; k < 16; ++k) v[k] = g_compile_ns[k].exchange(0);
    if (std::getenv("VQ_TIMING_SUB")) {
        std::fprintf(stderr, "[vq timing] inside 1:n resolve (thread-ms; 6 value-id gather, 7 sort, 8 pairs, 9 order check + layers):");
        for (int k = 6; k < 10; ++k) std::fprintf(stderr, " [%d] %.3f", k, v[k] * 1e-6);
        std::fprintf(stderr, "\n");
    }
    std::fprintf(stderr, "[vq timing] compile thread-ms: total %.3f = dictionary lookups %.3f + 1:n resolve %.3f + 1:n layers %.3f + leaf lists %.3f + rest %.3f; longest request %.3f\n", v[5] * 1e-6,
                 v[0] * 1e-6, v[1] * 1e-6, (v[2] - v[1]) * 1e-6, v[3] * 1e-6, (double(v[5]) - double(v[0]) - double(v[2]) - double(v[3])) * 1e-6, v[4] * 1e-6);
}

std::unique_ptr<PartialBatch> run_partial(const Index& idx, const vqreq::Request* const* reqs, size_t n, int slot, int64_t arena_offset) {
    const double t_start = now_ms();
    auto pb = std::make_unique<PartialBatch>();
    pb->index = &idx;
    pb->reqs.assign(reqs, reqs + n);
    pb->t0 = std::chrono::steady_clock::now();
    acquire_workspace(idx, *pb, slot);
    VQ_HIP(hipSetDevice(idx.device));
    Workspace& ws = *pb->ws;
    ws.timed.clear();
    ws.ev_used = 0;
    pb->profiled = idx.profile.enabled;

    const CompileReport compiled = compile_batch(idx, ws, *pb, reqs, n, idx.stream);
    size_spans(pb->queries);
    const BatchLayout layout = plan_layout(idx, *pb);
    const double t_layout = now_ms();
    const ScanPlan plan = pack_upload(idx, *pb, layout);
    if (layout.nq == 0) return pb;  // nothing compiled: there is nothing to launch (finish_batch reports the requests' errors)
    const double t_packed = now_ms();
    launch_scans(idx, *pb, layout, plan, arena_offset);
    report_timing(n, t_start, compiled, t_layout, t_packed, plan.tabs);
    return pb;
}

// One finished batch into the profile: the device time of every timed launch of the workspace under its kernel's entry (the caller holds
// profile_mutex, and the launches' stream has been synchronised)
static void account_timed_launches(Profile& P, Workspace& ws) {
    P.batches += 1;
    for (const TimedLaunch& t : ws.timed) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ws.ev_pool[t.ev_begin], ws.ev_pool[t.ev_end]) != hipSuccess) continue;
        KernelProfile& k = P.k[t.kernel];
        k.ms += ms;
        k.launches += 1;
        k.layout_bytes += t.layout_bytes;
        k.algorithmic_bytes += t.algorithmic_bytes;
        k.queries += t.queries;
    }
    ws.timed.clear();
}

// vq_debug_*_lists (capi.cpp): pre-pass drivers alone, on the next workspace in turn (held until `body` returns: the drivers' results live in
// it, `body` reads them back) and on the pre-passes' stream; their timed launches go to the profile like a batch's
void debug_prepass(const Index& idx, const std::function<void(Workspace&, hipStream_t)>& body) {
    VQ_HIP(hipSetDevice(idx.device));
    Workspace& ws = idx.ws[idx.next_ws.fetch_add(1) % kWorkspaces];
    std::unique_lock<std::mutex> lock(ws.mu);
    ws.timed.clear();
    ws.ev_used = 0;
    const hipStream_t st = idx.pre_stream ? idx.pre_stream : idx.stream;
    body(ws, st);
    VQ_HIP(hipStreamSynchronize(st));
    if (idx.profile.enabled) {
        std::lock_guard<std::mutex> g(idx.profile_mutex);
        account_timed_launches(idx.profile, ws);
    }
}

// The dictionary scans of a suggest / highlight request, answered: on the next workspace in turn, on the pre-passes' stream
static FuzzyTable run_suggest_probes(const Index& idx, const vqreq::Request& req) {
    FuzzyTable fuzzy;
    collect_suggest_probes(idx, req, fuzzy);
    if (fuzzy.empty()) return fuzzy;
    Workspace& ws = idx.ws[idx.next_ws.fetch_add(1) % kWorkspaces];
    std::unique_lock<std::mutex> lock(ws.mu);
    ws.timed.clear();
    ws.ev_used = 0;
    run_fuzzy_probes(idx, ws, fuzzy, idx.pre_stream ? idx.pre_stream : idx.stream);
    return fuzzy;
}

// suggest_multi (search_field.rs:194-219): dictionary side only — the parts' matched terms, equal texts merged keeping the best score, ranked
// (the merge over the parts, shared by the single request and the batch: `fuzzy` holds the answered scans of the request's parts)
static std::vector<SuggestEntry> merge_suggest_parts(const Index& idx, const vqreq::Request& req, const FuzzyTable& fuzzy, bool topn_probes = false) {
    std::vector<SuggestEntry> out;
    for (auto& part : *req.suggest) {
        auto one = suggest_part(idx, part, fuzzy.empty() ? nullptr : &fuzzy, topn_probes);
        out.insert(out.end(), one.begin(), one.end());
    }
    std::stable_sort(out.begin(), out.end(), [](const SuggestEntry& a, const SuggestEntry& b) { return a.text > b.text; });  // :176 (descending)
    std::vector<SuggestEntry> merged;
    for (auto& e : out) {
        if (!merged.empty() && merged.back().text == e.text) {
            if (e.score > merged.back().score) merged.back().score = e.score;
        } else merged.push_back(e);
    }
    std::stable_sort(merged.begin(), merged.end(), [](const SuggestEntry& a, const SuggestEntry& b) { return a.score > b.score; });  // :189
    const size_t skip = std::min(req.skip.value_or(0), merged.size());  // apply_top_skip, search.rs:230-239
    merged.erase(merged.begin(), merged.begin() + skip);
    if (req.top && merged.size() > *req.top) merged.resize(*req.top);
    return merged;
}
std::vector<SuggestEntry> run_suggest(const Index& idx, const vqreq::Request& req) {
    if (!req.suggest) throw VelociError(ERR_INVALID_REQUEST, "only suggest allowed in suggest function");
    VQ_HIP(hipSetDevice(idx.device));
    const FuzzyTable fuzzy = run_suggest_probes(idx, req);
    return merge_suggest_parts(idx, req, fuzzy);
}

// n suggest requests as one batch: the probes of ALL requests in one table (equal probes are scanned once), one run of the probe runner, then
// every request finished by the single request's own code.  A part with its own top gets a top-n probe where it qualifies (probe_part).
void run_suggest_batch(const Index& idx, const vqreq::Request* const* reqs, size_t n, std::vector<std::vector<SuggestEntry>>& out, std::vector<int>& status,
                       std::vector<std::string>& errors) {
    out.assign(n, {});
    status.assign(n, 0);
    errors.assign(n, std::string());
    if (!n) return;
    VQ_HIP(hipSetDevice(idx.device));
    FuzzyTable fuzzy;
    for (size_t i = 0; i < n; ++i) {
        if (!reqs[i]) {
            status[i] = vqreq::ERR_INVALID_ARGUMENT;
            errors[i] = "null request";
        } else if (!reqs[i]->suggest) {
            status[i] = ERR_INVALID_REQUEST;
            errors[i] = "only suggest allowed in suggest function";
        } else collect_suggest_batch_probes(idx, *reqs[i], fuzzy);
    }
    if (!fuzzy.empty()) {
        Workspace& ws = idx.ws[idx.next_ws.fetch_add(1) % kWorkspaces];
        std::unique_lock<std::mutex> lock(ws.mu);
        ws.timed.clear();
        ws.ev_used = 0;
        run_fuzzy_probes(idx, ws, fuzzy, idx.pre_stream ? idx.pre_stream : idx.stream);
        if (idx.profile.enabled) {  // (every launch of the runner is behind a host synchronisation)
            std::lock_guard<std::mutex> g(idx.profile_mutex);
            account_timed_launches(idx.profile, ws);
        }
        uint64_t topn = 0, records = 0;
        for (auto& kv : fuzzy) {
            if (kv.second.status != 0) continue;
            topn += kv.second.top_n != 0;
            records += kv.second.top_n ? kv.second.topn_copied : kv.second.matches.size();
        }
        idx.suggest_topn_probes.fetch_add(topn, std::memory_order_relaxed);
        idx.suggest_records_back.fetch_add(records, std::memory_order_relaxed);
    }
    parallel_for(n, std::min(host_threads(), n), [&](size_t i) {
        if (status[i] != 0) return;
        try {
            out[i] = merge_suggest_parts(idx, *reqs[i], fuzzy, true);
        } catch (const VelociError& e) {
            status[i] = e.code;
            errors[i] = e.what();
            out[i].clear();
        }
    });
}

// search_field::highlight (search_field.rs:233-245): the part's terms normalised (util.rs:11-29), its dictionary scan on the device, the snippets on
// the host, ranked by score with the part's own top / skip
static void rank_and_cut_highlight(std::vector<SuggestEntry>& out, const vqreq::RequestSearchPart& part) {
    std::stable_sort(out.begin(), out.end(), [](const SuggestEntry& a, const SuggestEntry& b) { return a.score > b.score; });  // :189
    const size_t skip = std::min(part.skip.value_or(0), out.size());  // apply_top_skip, search.rs:230-239
    out.erase(out.begin(), out.begin() + skip);
    if (part.top && out.size() > *part.top) out.resize(*part.top);
}
std::vector<SuggestEntry> run_highlight(const Index& idx, vqreq::RequestSearchPart part) {
    for (auto& t : part.terms) t = vqtext::normalize_text(t);
    VQ_HIP(hipSetDevice(idx.device));
    vqreq::Request probe_req;
    probe_req.suggest = std::vector<vqreq::RequestSearchPart>{part};
    const FuzzyTable fuzzy = run_suggest_probes(idx, probe_req);
    std::vector<SuggestEntry> out = highlight_part(idx, part, fuzzy.empty() ? nullptr : &fuzzy);
    rank_and_cut_highlight(out, part);
    return out;
}

// ---- the batched highlight: texts ranked and cut to the page on the device, snippets for the page only
namespace {
// VQ_NO_HIGHLIGHT_RANK=1: every part of a highlight batch keeps the host route
bool highlight_rank_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("VQ_NO_HIGHLIGHT_RANK");
        return !(e && *e && std::string(e) != "0");
    }();
    return on;
}

// The field's record, made on first use: do tokens_to_text_id and text_id_to_token_ids hold the same (token, text) pairs?  Then every text of
// a matched token's row has a token row that contains the token (it gets a snippet), and every matched token of a text's row lists the text
// (the text's hit tokens are its row's tokens inside the matched set).  A field that passes has the first table's values in HBM.
const Index::HighlightField& highlight_field(const Index& idx, const std::string& path) {
    Index::HighlightField* f;
    {
        std::lock_guard<std::mutex> g(idx.highlight_mu);
        auto& slot = idx.highlight_fields[path];
        if (!slot) slot = std::make_unique<Index::HighlightField>();
        f = slot.get();
    }
    std::call_once(f->once, [&] {
        auto a = idx.kv.find(path + TOKENS_TO_TEXT_ID), b = idx.kv.find(path + ".text_id_to_token_ids");
        if (a == idx.kv.end() || b == idx.kv.end()) return;
        const KVStore &t2t = a->second, &tokens = b->second;
        if (idx.sharded() && !t2t.text_csr) return;  // (only that case is known to keep the whole table on every shard)
        if (t2t.host_values.empty()) return;
        std::vector<uint64_t> p1, p2;  // token << 32 | text
        p1.reserve(t2t.host_values.size());
        p2.reserve(tokens.host_values.size());
        uint32_t max_text = 0;
        for (uint32_t r = 0; r < t2t.num_keys; ++r)
            for (uint64_t k = t2t.host_off[r]; k < t2t.host_off[r + 1]; ++k) {
                p1.push_back((uint64_t(t2t.key_base) + r) << 32 | t2t.host_values[k]);
                max_text = std::max(max_text, t2t.host_values[k]);
            }
        for (uint32_t r = 0; r < tokens.num_keys; ++r)
            for (uint64_t k = tokens.host_off[r]; k < tokens.host_off[r + 1]; ++k) p2.push_back(uint64_t(tokens.host_values[k]) << 32 | (uint64_t(tokens.key_base) + r));
        auto canon = [](std::vector<uint64_t>& v) {
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
        };
        parallel_for(2, std::min<size_t>(host_threads(), 2), [&](size_t i) { canon(i ? p2 : p1); });
        if (p1 != p2 || max_text == 0xFFFFFFFFu || (uint64_t(max_text) + 1) * 4 > kTextRankBudget) return;
        f->num_texts = max_text + 1;
        f->t2t = &t2t;
        f->tokens = &tokens;
        if (t2t.text_csr) f->d_vals = t2t.d_text_vals.as<uint32_t>();
        else {  // not staged by the index build (an identity field): now, once
            f->own_vals.alloc(t2t.host_values.size() * 4 + 16);
            f->own_vals.upload(t2t.host_values.data(), t2t.host_values.size() * 4);
            f->d_vals = f->own_vals.as<uint32_t>();
        }
        f->ok = true;
    });
    return *f;
}

struct TextRankSlot {
    uint32_t top_n = 0;
    std::vector<TextRowD> rows;                          // (slot filled in by the round)
    std::vector<std::pair<uint32_t, uint32_t>> picked;   // result: (text, score bits) sorted by (bits descending, text ascending)
    uint32_t touched = 0;                                // result: texts that hold a matched token
};
// the row of `len` values at `start` with score `bits`, in pieces of at most kTextRankSplit values
void add_text_rows(TextRankSlot& s, uint64_t start, uint64_t len, uint32_t bits) {
    for (uint64_t at = 0; at < len; at += kTextRankSplit) s.rows.push_back(TextRowD{start + at, uint32_t(std::min<uint64_t>(kTextRankSplit, len - at)), 0u, bits, 0u});
}
// k_text_best + k_text_select over `slots` of one table, in rounds whose `best` arrays fit kTextRankBudget; one download per round
void run_text_rank(bool timed, Workspace& ws, DevBuf& d_best, DevBuf& d_meta, hipStream_t st, const uint32_t* d_vals, uint32_t num_texts, std::vector<TextRankSlot*>& slots) {
    const size_t per_round = std::max<size_t>(1, kTextRankBudget / (size_t(num_texts) * 4));
    for (size_t s0 = 0; s0 < slots.size(); s0 += per_round) {
        const size_t ns = std::min(per_round, slots.size() - s0);
        std::vector<TextRowD> rows;
        std::vector<uint32_t> top_ns(ns);
        uint32_t stride = 1;
        uint64_t values = 0;
        for (size_t k = 0; k < ns; ++k) {
            TextRankSlot& S = *slots[s0 + k];
            if (S.top_n == 0 || S.top_n > kTextRankMaxTop) throw VelociError(ERR_DEVICE, "internal: a text-rank slot outside the kernels' range");
            top_ns[k] = S.top_n;
            stride = std::max(stride, S.top_n);
            for (TextRowD r : S.rows) {
                r.slot = uint32_t(k);
                values += r.len;
                rows.push_back(r);
            }
        }
        // tables: [rows][top_ns] up, [counts: 2 per slot][pairs: stride x 2 per slot] down
        const size_t top_at = align_up(rows.size() * sizeof(TextRowD), 256), down_at = top_at + align_up(ns * 4, 256), down_words = ns * 2 + ns * size_t(stride) * 2;
        d_meta.ensure(down_at + down_words * 4 + 16);
        d_best.ensure(ns * size_t(num_texts) * 4 + 16);
        uint8_t* meta = d_meta.as<uint8_t>();
        uint32_t* d_counts = reinterpret_cast<uint32_t*>(meta + down_at);
        if (!rows.empty()) VQ_HIP(hipMemcpyAsync(meta, rows.data(), rows.size() * sizeof(TextRowD), hipMemcpyHostToDevice, st));
        VQ_HIP(hipMemcpyAsync(meta + top_at, top_ns.data(), ns * 4, hipMemcpyHostToDevice, st));
        VQ_HIP(hipMemsetAsync(d_best.p, 0, ns * size_t(num_texts) * 4, st));
        {  // layout bytes: the row values read plus 4 B per atomic
            LaunchTimer timer(timed, ws, st, K_TEXT_BEST, values * 8, values * 8, ns);
            launch_text_best(st, reinterpret_cast<const TextRowD*>(meta), uint32_t(rows.size()), d_vals, num_texts, d_best.as<uint32_t>());
        }
        {  // num_texts x 4 B per pass over a slot's array: four radix passes, the count of the threshold's equals, the write
            LaunchTimer timer(timed, ws, st, K_TEXT_SELECT, uint64_t(ns) * num_texts * 4 * 6, uint64_t(ns) * num_texts * 4, ns);
            launch_text_select(st, d_best.as<uint32_t>(), num_texts, uint32_t(ns), reinterpret_cast<const uint32_t*>(meta + top_at), stride, d_counts, d_counts + 2 * ns);
        }
        VQ_HIP(hipGetLastError());
        std::vector<uint32_t> down(down_words);
        VQ_HIP(hipMemcpyAsync(down.data(), d_counts, down_words * 4, hipMemcpyDeviceToHost, st));
        VQ_HIP(hipStreamSynchronize(st));
        for (size_t k = 0; k < ns; ++k) {
            TextRankSlot& S = *slots[s0 + k];
            const uint32_t n = down[2 * k];
            S.touched = down[2 * k + 1];
            if (n > S.top_n || n > S.touched) throw VelociError(ERR_DEVICE, "text rank: more pairs than the slot asked for");
            const uint32_t* pairs = down.data() + 2 * ns + k * size_t(stride) * 2;
            S.picked.resize(n);
            for (uint32_t j = 0; j < n; ++j) S.picked[j] = {pairs[2 * j], pairs[2 * j + 1]};
            std::sort(S.picked.begin(), S.picked.end(), [](auto& a, auto& b) { return a.second != b.second ? a.second > b.second : a.first < b.first; });
        }
    }
}
}  // namespace

void debug_text_rank(const uint64_t* row_off, const uint32_t* vals, const uint32_t* bits, uint32_t num_rows, uint32_t num_texts, uint32_t top_n,
                     std::vector<std::pair<uint32_t, uint32_t>>& picked, uint32_t* touched) {
    Workspace ws;  // (untimed: only handed through)
    DevBuf d_vals, d_best, d_meta;
    const uint64_t n_vals = num_rows ? row_off[num_rows] : 0;
    d_vals.alloc(n_vals * 4 + 16);
    if (n_vals) d_vals.upload(vals, n_vals * 4);
    TextRankSlot slot;
    slot.top_n = top_n;
    for (uint32_t r = 0; r < num_rows; ++r) add_text_rows(slot, row_off[r], row_off[r + 1] - row_off[r], bits[r]);
    std::vector<TextRankSlot*> slots{&slot};
    run_text_rank(false, ws, d_best, d_meta, nullptr, d_vals.as<uint32_t>(), num_texts, slots);
    picked = std::move(slot.picked);
    *touched = slot.touched;
}

void run_highlight_batch(const Index& idx, const vqreq::RequestSearchPart* const* parts_in, size_t n, std::vector<std::vector<SuggestEntry>>& out, std::vector<int>& status,
                         std::vector<std::string>& errors) {
    out.assign(n, {});
    status.assign(n, 0);
    errors.assign(n, std::string());
    if (!n) return;
    VQ_HIP(hipSetDevice(idx.device));
    // the parts with their terms normalised (search_field.rs:234), and the dictionary scans of all of them in one table
    std::vector<vqreq::RequestSearchPart> parts(n);
    vqreq::Request probe_req;
    probe_req.suggest = std::vector<vqreq::RequestSearchPart>();
    for (size_t i = 0; i < n; ++i) {
        if (!parts_in[i]) {
            status[i] = vqreq::ERR_INVALID_ARGUMENT;
            errors[i] = "null request";
            continue;
        }
        parts[i] = *parts_in[i];
        for (auto& t : parts[i].terms) t = vqtext::normalize_text(t);
        probe_req.suggest->push_back(parts[i]);
    }
    FuzzyTable fuzzy;
    collect_suggest_probes(idx, probe_req, fuzzy);
    Workspace& ws = idx.ws[idx.next_ws.fetch_add(1) % kWorkspaces];
    std::unique_lock<std::mutex> lock(ws.mu);
    ws.timed.clear();
    ws.ev_used = 0;
    hipStream_t st = idx.pre_stream ? idx.pre_stream : idx.stream;
    if (!fuzzy.empty()) run_fuzzy_probes(idx, ws, fuzzy, st);
    auto fail = [&](size_t i, const VelociError& e) {
        status[i] = e.code;
        errors[i] = e.what();
        out[i].clear();
    };
    // every part's matched tokens, by the single call's own code
    std::vector<HighlightLookup> looked(n);
    std::vector<uint8_t> on_device(n, 0);
    const size_t threads = std::min(host_threads(), n);
    parallel_for(n, threads, [&](size_t i) {
        if (status[i] != 0) return;
        try {
            looked[i] = highlight_lookup(idx, parts[i], fuzzy.empty() ? nullptr : &fuzzy);
        } catch (const VelociError& e) {
            return fail(i, e);
        }
        const vqreq::RequestSearchPart& p = parts[i];
        const HighlightLookup& lk = looked[i];
        bool ok = highlight_rank_enabled() && lk.tokenized && lk.add_snippets && p.top && !lk.hits_scores.empty() && *p.top <= kTextRankMaxTop &&
                  p.skip.value_or(0) <= kTextRankMaxTop && *p.top + p.skip.value_or(0) >= 1 && *p.top + p.skip.value_or(0) <= kTextRankMaxTop;
        for (auto& h : lk.hits_scores) ok = ok && std::isfinite(h.second) && h.second > 0.0f;
        on_device[i] = ok;
    });
    // the device parts: the field's record (the store check and the staging happen here, on this thread), one slot per distinct part
    std::map<std::string, std::vector<TextRankSlot*>> by_field;
    std::map<std::string, std::unique_ptr<TextRankSlot>> slot_of_key;
    std::vector<TextRankSlot*> slot_of_part(n, nullptr);
    for (size_t i = 0; i < n; ++i) {
        if (status[i] != 0 || !on_device[i]) continue;
        const HighlightLookup& lk = looked[i];
        const Index::HighlightField& f = highlight_field(idx, lk.path);
        if (!f.ok) {
            on_device[i] = 0;
            continue;
        }
        const uint32_t top_n = uint32_t(*parts[i].top + parts[i].skip.value_or(0));
        std::string key = lk.path;
        key.push_back('\0');
        key.append(reinterpret_cast<const char*>(&top_n), 4);
        key.append(reinterpret_cast<const char*>(lk.hits_scores.data()), lk.hits_scores.size() * sizeof(lk.hits_scores[0]));
        auto& slot = slot_of_key[key];
        if (!slot) {
            slot = std::make_unique<TextRankSlot>();
            slot->top_n = top_n;
            for (auto& h : lk.hits_scores) {
                if (h.first < f.t2t->key_base || h.first - f.t2t->key_base >= f.t2t->num_keys) continue;  // (KVStore::host_row: no row)
                const uint32_t r = h.first - f.t2t->key_base;
                uint32_t bits;
                std::memcpy(&bits, &h.second, 4);
                add_text_rows(*slot, f.t2t->host_off[r], f.t2t->host_off[r + 1] - f.t2t->host_off[r], bits);
            }
            by_field[lk.path].push_back(slot.get());
        }
        slot_of_part[i] = slot.get();
    }
    for (auto& [path, slots] : by_field) {
        const Index::HighlightField& f = highlight_field(idx, path);
        run_text_rank(idx.profile.enabled, ws, ws.d_trank_best, ws.d_trank_meta, st, f.d_vals, f.num_texts, slots);
    }
    if (idx.profile.enabled) {  // (every launch above is behind a host synchronisation)
        std::lock_guard<std::mutex> g(idx.profile_mutex);
        account_timed_launches(idx.profile, ws);
    }
    lock.unlock();
    // finish: a device part sorts nothing more — its slot is ranked — and builds the page's snippets; every other part takes the host route
    std::atomic<uint64_t> device_parts{0}, snippets{0};
    parallel_for(n, threads, [&](size_t i) {
        if (status[i] != 0) return;
        const vqreq::RequestSearchPart& p = parts[i];
        const HighlightLookup& lk = looked[i];
        try {
            const TextRankSlot* S = slot_of_part[i];
            bool done = false;
            if (S && S->touched != 0) {  // (no touched text: the host route answers that case, or fails as the single call does)
                std::vector<uint32_t> wanted;
                for (auto& h : lk.hits_scores) wanted.push_back(h.first);
                std::sort(wanted.begin(), wanted.end());
                const size_t skip = std::min<size_t>(p.skip.value_or(0), S->picked.size());
                const size_t end = std::min<size_t>(S->picked.size(), skip + *p.top);
                done = true;
                for (size_t k = skip; k < end && done; ++k) {
                    SuggestEntry e;
                    e.term_id = S->picked[k].first;
                    std::memcpy(&e.score, &S->picked[k].second, 4);
                    done = highlight_snippet(idx, lk, p, e.term_id, wanted, &e.text);  // (the store check rules a miss out)
                    out[i].push_back(std::move(e));
                }
                if (done) {
                    device_parts.fetch_add(1, std::memory_order_relaxed);
                    snippets.fetch_add(out[i].size(), std::memory_order_relaxed);
                } else out[i].clear();
            }
            if (!done) {
                out[i] = highlight_resolve(idx, p, lk);
                snippets.fetch_add(out[i].size(), std::memory_order_relaxed);  // (one per text that holds a matched token)
                rank_and_cut_highlight(out[i], p);
            }
        } catch (const VelociError& e) {
            fail(i, e);
        }
    });
    idx.highlight_device_parts.fetch_add(device_parts.load(), std::memory_order_relaxed);
    idx.highlight_snippets_built.fetch_add(snippets.load(), std::memory_order_relaxed);
}

// The continuation of a request behind the ranked hit (score, id): the next kMaxTopK hits below that key, no facets (page 0 counted them)
vqreq::Request page_request_after(const vqreq::Request& R, float score, uint32_t id) {
    vqreq::Request page = R;
    page.top = size_t(kMaxTopK);
    page.skip = 0;
    page.facets.reset();
    uint32_t bits;
    std::memcpy(&bits, &score, 4);
    page.key_upper = (uint64_t(order_f32(bits)) << 32) | id;
    return page;
}

void complete_deep_requests(const Index& idx, const vqreq::Request* const* reqs, size_t n, std::vector<std::unique_ptr<Result>>& results,
                            std::vector<int>& status, std::vector<std::string>& errors) {
    constexpr uint64_t kMaxDeep = 65536;  // ranked hits one request may reach (64 scans)
    for (size_t i = 0; i < n; ++i) {
        if (status[i] != 0 || !results[i] || !results[i]->deep) continue;
        const vqreq::Request& R = *reqs[i];
        Result& out = *results[i];
        out.deep = false;
        const uint64_t top = R.top.value_or(10), skip = R.skip.value_or(0);
        const uint64_t want = top + skip < top ? ~0ull : top + skip;
        std::vector<uint32_t> ids = std::move(out.ids);  // page 0: the best kMaxTopK
        std::vector<float> scores = std::move(out.scores);
        out.ids.clear();
        out.scores.clear();
        if (skip >= out.num_hits) continue;  // apply_top_skip (search.rs:230-239): nothing left behind the skipped hits
        const uint64_t reach = std::min<uint64_t>(want, out.num_hits);
        if (reach > kMaxDeep) {
            status[i] = ERR_UNSUPPORTED;
            errors[i] = "unsupported on the MI355X query path: top + skip reaches more than " + std::to_string(kMaxDeep) + " ranked hits";
            results[i].reset();
            continue;
        }
        vqreq::Request page = R;
        page.top = size_t(kMaxTopK);
        page.skip = 0;
        page.facets.reset();  // (counted by page 0)
        bool failed = false;
        while (ids.size() < reach && ids.size() % size_t(kMaxTopK) == 0 && !ids.empty()) {
            uint32_t bits;
            std::memcpy(&bits, &scores.back(), 4);
            page.key_upper = (uint64_t(order_f32(bits)) << 32) | ids.back();
            const vqreq::Request* arr[1] = {&page};
            std::vector<std::unique_ptr<Result>> r;
            std::vector<int> st;
            std::vector<std::string> er;
            {
                auto pb = run_partial(idx, arr, 1);
                finish_batch(idx, *pb, nullptr, 1, r, st, er);
            }
            if (st[0] != 0) {
                status[i] = st[0];
                errors[i] = er[0];
                results[i].reset();
                failed = true;
                break;
            }
            if (r[0]->ids.empty()) break;
            ids.insert(ids.end(), r[0]->ids.begin(), r[0]->ids.end());
            scores.insert(scores.end(), r[0]->scores.begin(), r[0]->scores.end());
        }
        if (failed) continue;
        const size_t from = size_t(std::min<uint64_t>(skip, ids.size())), to = size_t(std::min<uint64_t>(want, ids.size()));
        out.ids.assign(ids.begin() + from, ids.begin() + to);
        out.scores.assign(scores.begin() + from, scores.begin() + to);
    }
}

// ---- explain: Explain records of the returned hits.  k_explain recomputes each hit's score through the request's tree and
// writes every value the records quote; what follows here is the reference's bookkeeping of WHICH records a hit collects, in which order.
std::string explain_records_json(const ExplainRecs& records) {  // serde's externally tagged enum (explain.rs:1-21), floats as %.9g (round-trips f32)
    auto f = [](float v) {
        char buf[48];
        std::snprintf(buf, sizeof buf, "%.9g", double(v));
        return std::string(buf);
    };
    std::string out = "[";
    for (size_t i = 0; i < records.size(); ++i) {
        const ExplainRec& e = records[i];
        if (i) out += ",";
        switch (e.kind) {
            case ExplainRec::Boost: out += "{\"Boost\":" + f(e.a) + "}"; break;
            case ExplainRec::MaxTokenToTextId: out += "{\"MaxTokenToTextId\":" + f(e.a) + "}"; break;
            case ExplainRec::OrSumOverDistinctTerms: out += "{\"OrSumOverDistinctTerms\":" + f(e.a) + "}"; break;
            case ExplainRec::TermToAnchor:
                out += "{\"TermToAnchor\":{\"term_score\":" + f(e.a) + ",\"anchor_score\":" + f(e.b) + ",\"final_score\":" + f(e.c) + ",\"term_id\":" + std::to_string(e.term_id) + "}}";
                break;
            case ExplainRec::LevenshteinScore:
                out += "{\"LevenshteinScore\":{\"score\":" + f(e.a) + ",\"text_or_token_id\":";
                vqjson::escape_to(out, e.text);
                out += ",\"term_id\":" + std::to_string(e.term_id) + "}}";
                break;
        }
    }
    return out + "]";
}

namespace {
struct ExplainEval {
    bool has = false;  // the node's explain map holds an entry for the doc
    ExplainRecs recs;
};
inline float trace_f32(uint32_t bits) {
    float v;
    std::memcpy(&v, &bits, 4);
    return v;
}
// The explain map entry of `doc` in the result of `node` — leaf: search_field.rs:419-441 on top of field_result.rs:44; and: set_op.rs:421-433;
// or: set_op.rs:132-137, 187-208.
ExplainEval explain_node(const ExplainPlan& P, int node, uint32_t doc, const uint32_t* T) {
    const ExplainNode& n = P.nodes[size_t(node)];
    ExplainEval out;
    if (n.kind == XP_LEAF) {
        auto stray = n.term_records.find(doc);  // new_from() copied the dictionary result's map: `doc` may be one of its TERM ids
        if (stray != n.term_records.end()) {
            out.has = true;
            out.recs = stray->second;
        }
        for (uint32_t j = 0; j < n.list_count; ++j) {
            const uint32_t* t = T + 3u * (n.list_begin + j);
            if (t[0] == 0xFFFFFFFFu) continue;
            out.has = true;
            ExplainRec e;
            e.kind = ExplainRec::TermToAnchor;
            e.term_id = n.list_term[j];
            e.a = P.lists[n.list_begin + j].term_score;
            e.b = trace_f32(t[1]);
            e.c = trace_f32(t[2]);
            out.recs.push_back(e);
            auto tr = n.term_records.find(n.list_term[j]);
            if (tr != n.term_records.end()) out.recs.insert(out.recs.end(), tr->second.begin(), tr->second.end());
        }
        return out;
    }
    const uint32_t* t_op = T + 3u * uint32_t(P.lists.size()) + 3u * uint32_t(n.op);
    const bool present = t_op[0] != 0;
    if (n.kind == XP_AND) {
        if (!present) return out;  // the result's map only has entries of its hits
        for (size_t k = 0; k + 1 < n.order.size(); ++k) {  // the operands left after the shortest one was taken out, in their new order (:393)
            ExplainEval c = explain_node(P, n.children[n.order[k]], doc, T);
            if (!c.has) continue;
            out.has = true;
            out.recs.insert(out.recs.end(), c.recs.begin(), c.recs.end());
        }
        return out;
    }
    std::vector<ExplainEval> ch;
    for (int c : n.children) ch.push_back(explain_node(P, c, doc, T));
    for (auto& c : ch)
        if (c.has) {  // HashMap::extend (:135): a later operand's entry replaces an earlier one's
            out.has = true;
            out.recs = c.recs;
        }
    if (present) {
        out.has = true;
        ExplainRec e;
        e.kind = ExplainRec::OrSumOverDistinctTerms;
        e.a = trace_f32(t_op[2]);
        out.recs.push_back(e);
        for (auto& c : ch)
            if (c.has) out.recs.insert(out.recs.end(), c.recs.begin(), c.recs.end());
    }
    return out;
}
}  // namespace

void complete_explain_requests(const Index& idx, std::vector<std::unique_ptr<Result>>& results, std::vector<int>& status, std::vector<std::string>& errors) {
    std::vector<ExQuery> queries;
    std::vector<size_t> owner;
    std::vector<uint32_t> doc_query, docs;
    std::vector<ExOp> ops;
    std::vector<uint16_t> aux;
    std::vector<ExList> lists;
    std::vector<DColBoost> cols;
    size_t trace_words = 0;
    for (size_t i = 0; i < results.size(); ++i) {
        if (status[i] != 0 || !results[i] || !results[i]->explain_plan) continue;
        Result& R = *results[i];
        const ExplainPlan& P = *R.explain_plan;
        R.has_explain = true;
        R.explain.assign(R.ids.size(), {});
        if (R.ids.empty()) continue;
        ExQuery q{};
        q.op_begin = uint32_t(ops.size());
        q.n_ops = uint32_t(P.ops.size());
        q.list_begin = uint32_t(lists.size());
        q.n_lists = uint32_t(P.lists.size());
        q.col_begin = uint32_t(cols.size());
        q.n_col = uint32_t(P.cols.size());
        q.doc_begin = uint32_t(docs.size());
        q.trace_begin = uint32_t(trace_words);
        for (ExOp op : P.ops) {
            if (op.kind != XP_LEAF) op.a += uint32_t(aux.size());
            ops.push_back(op);
        }
        aux.insert(aux.end(), P.aux.begin(), P.aux.end());
        lists.insert(lists.end(), P.lists.begin(), P.lists.end());
        cols.insert(cols.end(), P.cols.begin(), P.cols.end());
        docs.insert(docs.end(), R.ids.begin(), R.ids.end());
        doc_query.insert(doc_query.end(), R.ids.size(), uint32_t(queries.size()));
        trace_words += R.ids.size() * size_t(explain_trace_words(q.n_lists, q.n_ops, q.n_col));
        if (trace_words > (1ull << 30)) {
            status[i] = ERR_UNSUPPORTED;
            errors[i] = "unsupported on the MI355X query path: explain trace of more than 4 GiB";
            results[i].reset();
            return;
        }
        queries.push_back(q);
        owner.push_back(i);
    }
    if (docs.empty()) return;
    VQ_HIP(hipSetDevice(idx.device));
    // one upload area: [queries][doc_query][docs][ops][aux][lists][cols], then the trace
    size_t off = 0;
    auto place = [&](size_t bytes) {
        const size_t at = off;
        off = align_up(off + bytes, 64);
        return at;
    };
    const size_t o_q = place(queries.size() * sizeof(ExQuery)), o_dq = place(doc_query.size() * 4), o_d = place(docs.size() * 4), o_ops = place(ops.size() * sizeof(ExOp)),
                 o_aux = place(aux.size() * 2), o_l = place(lists.size() * sizeof(ExList)), o_c = place(cols.size() * sizeof(DColBoost));
    std::vector<uint8_t> up(off);
    std::memcpy(up.data() + o_q, queries.data(), queries.size() * sizeof(ExQuery));
    std::memcpy(up.data() + o_dq, doc_query.data(), doc_query.size() * 4);
    std::memcpy(up.data() + o_d, docs.data(), docs.size() * 4);
    std::memcpy(up.data() + o_ops, ops.data(), ops.size() * sizeof(ExOp));
    if (!aux.empty()) std::memcpy(up.data() + o_aux, aux.data(), aux.size() * 2);
    if (!lists.empty()) std::memcpy(up.data() + o_l, lists.data(), lists.size() * sizeof(ExList));
    if (!cols.empty()) std::memcpy(up.data() + o_c, cols.data(), cols.size() * sizeof(DColBoost));
    DevBuf d_up, d_trace;
    d_up.ensure(off);
    d_trace.ensure(trace_words * 4);
    hipStream_t st = idx.stream;
    VQ_HIP(hipMemcpyAsync(d_up.p, up.data(), off, hipMemcpyHostToDevice, st));
    const uint8_t* du = d_up.as<uint8_t>();
    launch_explain(st, uint32_t(docs.size()), reinterpret_cast<const ExQuery*>(du + o_q), reinterpret_cast<const uint32_t*>(du + o_dq), reinterpret_cast<const uint32_t*>(du + o_d),
                   reinterpret_cast<const ExOp*>(du + o_ops), reinterpret_cast<const uint16_t*>(du + o_aux), reinterpret_cast<const ExList*>(du + o_l),
                   reinterpret_cast<const DColBoost*>(du + o_c), d_trace.as<uint32_t>());
    VQ_HIP(hipGetLastError());
    std::vector<uint32_t> trace(trace_words);
    VQ_HIP(hipMemcpyAsync(trace.data(), d_trace.p, trace_words * 4, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    for (size_t k = 0; k < queries.size(); ++k) {
        const ExQuery& q = queries[k];
        Result& R = *results[owner[k]];
        const ExplainPlan& P = *R.explain_plan;
        const uint32_t words = explain_trace_words(q.n_lists, q.n_ops, q.n_col);
        for (size_t h = 0; h < R.ids.size(); ++h) {
            const uint32_t* T = trace.data() + q.trace_begin + h * size_t(words);
            const uint32_t* t_cols = T + 3u * (q.n_lists + q.n_ops);
            if (t_cols[3u * q.n_col] == 0) {  // a returned hit is a hit of the tree
                status[owner[k]] = ERR_UNSUPPORTED;
                errors[owner[k]] = "internal: explain did not reproduce hit " + std::to_string(R.ids[h]);
                break;
            }
            ExplainEval e = explain_node(P, P.root, R.ids[h], T);
            for (uint32_t c = 0; c < q.n_col; ++c) {  // add_boost (boost.rs:470-504) -> apply_boost's records (:297-300, :371-374)
                if (t_cols[3u * c] == 0) continue;
                e.has = true;
                ExplainRec b;
                b.kind = ExplainRec::Boost;
                if (P.cols[c].fun == BF_LOG10) {
                    b.a = trace_f32(t_cols[3u * c + 1u]);
                    e.recs.push_back(b);
                }
                b.a = trace_f32(t_cols[3u * c + 2u]);
                e.recs.push_back(b);
            }
            R.explain[h] = {e.has, std::move(e.recs)};
        }
        if (status[owner[k]] != 0) results[owner[k]].reset();
    }
}

PartialBatch::~PartialBatch() {
    if (ws && launched && !finished && ws->ev_done) (void)hipEventSynchronize(ws->ev_done);
    release_workspace();
}
// the workspace goes back: a batch that named it takes its mark off FIRST (a workspace that stayed marked would be skipped by every later
// batch — and four of those left an index without workspaces)
void PartialBatch::release_workspace() {
    if (!lock.owns_lock()) return;
    if (ws && pinned_ws) {
        ws->pinned.store(false, std::memory_order_release);
        pinned_ws = false;
    }
    lock.unlock();
}

namespace {
struct DownLayout {  // download area: [hits u64 nq][n u32 nq][ids u32 K][scores f32 K][facet_n u32 J][facet_vals u32 F][facet_counts u32 F]
    size_t K, J, F, o_hits, o_n, o_ids, o_scores, o_fn, o_fv, o_fc, o_stat, bytes;
    explicit DownLayout(const PartialBatch& pb) {
        const uint32_t nq = pb.nq_dev;
        K = size_t(pb.layout.total_keys);
        J = pb.n_facet_jobs;
        F = pb.total_facet_out;
        o_hits = 0;
        o_n = align_up(o_hits + size_t(nq) * 8, 16);
        o_ids = align_up(o_n + size_t(nq) * 4, 16);
        o_scores = align_up(o_ids + K * 4, 16);
        o_fn = align_up(o_scores + K * 4, 16);
        o_fv = align_up(o_fn + J * 4, 16);
        o_fc = align_up(o_fv + F * 4, 16);
        o_stat = align_up(o_fc + F * 4, 16);  // profiling: gathered bytes per query (its own copy, straight into the pinned area)
        bytes = align_up(o_stat + size_t(nq) * 8, 256);
    }
};
}  // namespace

void finish_launch(const Index& idx, PartialBatch& pb, const void* gathered_device, uint32_t num_shards, size_t shard_stride) {
    if (pb.merge_launched) return;
    pb.merge_launched = true;
    Workspace& ws = *pb.ws;
    hipStream_t st = idx.fin_stream;
    const PartialLayout& lay = pb.layout;
    const uint32_t nq = pb.nq_dev;
    VQ_HIP(hipSetDevice(idx.device));
    const DownLayout D(pb);
    const size_t K = D.K, J = D.J;
    if (!nq) return;
    const uint8_t* gathered = gathered_device ? static_cast<const uint8_t*>(gathered_device) : pb.d_partial;
    if (!gathered_device) num_shards = 1;
    ws.d_down.ensure(D.bytes);
    ws.h_down.ensure(D.bytes);
    if (st != idx.stream) VQ_HIP(hipStreamWaitEvent(st, ws.ev_done, 0));
    uint8_t* dd = ws.d_down.as<uint8_t>();
    const bool prof = pb.profiled;
    {
        LaunchTimer t(prof, ws, st, K_FINALIZE, uint64_t(num_shards) * (K * 8 + nq * 8) + K * 8, uint64_t(num_shards) * (K * 8 + nq * 8) + K * 8, nq);
        launch_finalize(st, nq, pb.d_blobs, pb.d_blob_off, gathered, num_shards, shard_stride ? shard_stride : size_t(lay.off_hist), lay, reinterpret_cast<uint32_t*>(dd + D.o_ids),
                        reinterpret_cast<float*>(dd + D.o_scores), reinterpret_cast<uint32_t*>(dd + D.o_n), reinterpret_cast<unsigned long long*>(dd + D.o_hits));
    }
    VQ_HIP(hipGetLastError());
    if (J) {
        // the batch's own histogram area: the caller of the sharded path has summed it over the shards in place (all-reduce)
        const uint32_t* hist = reinterpret_cast<const uint32_t*>(pb.d_partial + lay.off_hist);
        LaunchTimer t(prof, ws, st, K_FACET_SELECT, lay.total_hist * 4, lay.total_hist * 4, J);
        launch_facet_select(st, uint32_t(J), pb.d_facet_jobs, hist, reinterpret_cast<uint32_t*>(dd + D.o_fv), reinterpret_cast<uint32_t*>(dd + D.o_fc),
                            reinterpret_cast<uint32_t*>(dd + D.o_fn));
        VQ_HIP(hipGetLastError());
    }
    VQ_HIP(hipMemcpyAsync(ws.h_down.p, dd, D.o_stat, hipMemcpyDeviceToHost, st));
    if (prof)  // bytes the scans read through per-hit gathers (counted by the kernels), per query — into PINNED memory: a copy into pageable memory
               // would hold this thread until the stream gets there
        VQ_HIP(hipMemcpyAsync(ws.h_down.as<uint8_t>() + D.o_stat, pb.d_partial + lay.off_stats, size_t(nq) * 8, hipMemcpyDeviceToHost, st));
}

void finish_batch(const Index& idx, PartialBatch& pb, const void* gathered_device, uint32_t num_shards, std::vector<std::unique_ptr<Result>>& out,
                  std::vector<int>& status, std::vector<std::string>& errors, size_t shard_stride) {
    const size_t n = pb.queries.size();
    out.clear();
    out.resize(n);
    status.assign(n, 0);
    errors.assign(n, std::string());
    finish_launch(idx, pb, gathered_device, num_shards, shard_stride);
    Workspace& ws = *pb.ws;
    hipStream_t st = idx.fin_stream;
    const PartialLayout& lay = pb.layout;
    const uint32_t nq = pb.nq_dev;
    const DownLayout D(pb);
    const size_t o_hits = D.o_hits, o_n = D.o_n, o_ids = D.o_ids, o_scores = D.o_scores, o_fn = D.o_fn, o_fv = D.o_fv, o_fc = D.o_fc;
    if (nq) {
        const bool prof = pb.profiled;
        VQ_HIP(hipStreamSynchronize(st));
        const uint64_t* gathered_bytes = reinterpret_cast<const uint64_t*>(ws.h_down.as<uint8_t>() + D.o_stat);
        pb.finished = true;
        if (prof) {
            std::lock_guard<std::mutex> g(idx.profile_mutex);
            Profile& P = idx.profile;
            account_timed_launches(P, ws);
            for (uint32_t q = 0; q < nq && q < pb.qclass.size(); ++q) {
                P.k[pb.qclass[q]].layout_bytes += gathered_bytes[q];
                P.k[pb.qclass[q]].gathered_bytes += gathered_bytes[q];
            }
        }
    }
    const uint64_t ns = uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - pb.t0).count());
    const double t_synced = now_ms();

    const uint8_t* hd = ws.h_down.as<uint8_t>();
    size_t key_off = 0, job = 0, fac_off = 0;
    for (size_t i = 0; i < n; ++i) {
        const CompiledQuery& cq = pb.queries[i];
        if (cq.status != 0) {
            status[i] = cq.status;
            errors[i] = cq.error;
            continue;
        }
        const uint32_t q = pb.slot[i];
        auto r = std::make_unique<Result>();
        r->num_hits = reinterpret_cast<const uint64_t*>(hd + o_hits)[q];
        r->execution_time_ns = ns;
        const uint32_t have = reinterpret_cast<const uint32_t*>(hd + o_n)[q];
        const uint32_t* ids = reinterpret_cast<const uint32_t*>(hd + o_ids) + key_off;
        const float* scores = reinterpret_cast<const float*>(hd + o_scores) + key_off;
        // apply_top_skip (search.rs:230-239) on the top+skip window
        const uint32_t want = cq.top + cq.skip;
        const uint32_t avail = std::min(have, want);
        const uint32_t from = std::min(cq.skip, avail);
        const uint32_t to = std::min(avail, from + cq.top);
        r->ids.assign(ids + from, ids + to);
        r->scores.assign(scores + from, scores + to);
        r->deep = cq.deep;
        if (!std::isnan(cq.or_skip_bound)) {
            // k_scan_probe_or ranked only the docs that hold the OR's cover operand.  Nothing was missed if every hit holds it, or if the last key of
            // the ranked window lies above what a doc WITHOUT the cover can score at best
            const bool confirmed = r->num_hits == have || (have == cq.top_k && cq.top_k > 0 && scores[cq.top_k - 1] > cq.or_skip_bound);
            r->rerun_exact = !confirmed;
        }
        key_off += cq.top_k;
        if (!cq.facet_out.empty()) r->has_facets = true;
        r->why_found_terms = cq.why_found_terms;
        r->explain_plan = cq.explain_plan;
        r->why_found_plan = cq.why_found_plan;
        for (size_t f = 0; f < cq.facet_out.size(); ++f, ++job) {
            const FacetOut& fo = cq.facet_out[f];
            ResultFacet rf;
            rf.field = fo.field;
            const uint32_t fn = reinterpret_cast<const uint32_t*>(hd + o_fn)[job];
            // jobs were appended in query order: this job's output offset is the running sum of the tops
            const auto dit = idx.dict.find(fo.dict_path);
            const size_t out_off = fac_off;
            fac_off += fo.top;
            const uint32_t* fv = reinterpret_cast<const uint32_t*>(hd + o_fv) + out_off;
            const uint32_t* fc = reinterpret_cast<const uint32_t*>(hd + o_fc) + out_off;
            for (uint32_t k = 0; k < fn && k < fo.top; ++k) {
                std::string text = (dit != idx.dict.end() && fv[k] < dit->second.terms.size()) ? dit->second.terms[fv[k]] : std::string();
                rf.entries.push_back({std::move(text), uint64_t(fc[k])});
            }
            if (fo.host_top) {  // more entries than the device ranks: the job's counts (summed over the shards in place), ranked here — count descending,
                                // value id ascending like k_facet_select (the reference's sort is unstable, facet.rs:19-23)
                const FacetJob& fj = pb.facet_jobs[job];
                std::vector<uint32_t> counts(fj.num_values);
                VQ_HIP(hipMemcpyAsync(counts.data(), pb.d_partial + lay.off_hist + size_t(fj.hist_off) * 4, size_t(fj.num_values) * 4, hipMemcpyDeviceToHost, st));
                VQ_HIP(hipStreamSynchronize(st));
                std::vector<uint32_t> order;
                for (uint32_t v = 0; v < fj.num_values; ++v)
                    if (counts[v]) order.push_back(v);
                const size_t keep = std::min<size_t>(order.size(), fo.host_top);
                std::partial_sort(order.begin(), order.begin() + keep, order.end(), [&](uint32_t x, uint32_t y) { return counts[x] != counts[y] ? counts[x] > counts[y] : x < y; });
                for (size_t k = 0; k < keep; ++k) {
                    std::string text = (dit != idx.dict.end() && order[k] < dit->second.terms.size()) ? dit->second.terms[order[k]] : std::string();
                    rf.entries.push_back({std::move(text), uint64_t(counts[order[k]])});
                }
            }
            r->facets.push_back(std::move(rf));
        }
        out[i] = std::move(r);
    }
    pb.release_workspace();
    {  // requests whose speculative route could not be confirmed run again, as a batch of their own, on the exact routes (rare: an OR whose best
       // hits lack its rarest term, or fewer such hits than the request asks for)
        std::vector<size_t> redo;
        for (size_t i = 0; i < n; ++i)
            if (out[i] && out[i]->rerun_exact) redo.push_back(i);
        if (!redo.empty()) {
            std::vector<vqreq::Request> again;
            again.reserve(redo.size());
            for (size_t i : redo) {
                again.push_back(*pb.reqs[i]);
                again.back().exact_routes_only = true;
            }
            std::vector<const vqreq::Request*> arr;
            for (auto& a : again) arr.push_back(&a);
            std::vector<std::unique_ptr<Result>> r2;
            std::vector<int> st2;
            std::vector<std::string> er2;
            {
                auto pb2 = run_partial(idx, arr.data(), arr.size());
                finish_batch(idx, *pb2, nullptr, 1, r2, st2, er2, 0);
            }
            for (size_t k = 0; k < redo.size(); ++k) {
                out[redo[k]] = std::move(r2[k]);
                status[redo[k]] = st2[k];
                errors[redo[k]] = er2[k];
            }
            idx.or_reruns.fetch_add(redo.size(), std::memory_order_relaxed);
        }
    }
    if (timing_enabled()) std::fprintf(stderr, "[vq timing] batch wall %.3f ms, result assembly %.3f ms\n", double(ns) * 1e-6, now_ms() - t_synced);
}

}  // namespace vq
