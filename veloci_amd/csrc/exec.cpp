// Batch executor: compile n requests, pack their device programs, launch the kernels, assemble results.
// One batch == one k_tile_scan launch over all (query, span) pairs (SURVEY.md §7 "design for batches").
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>

#include "engine.hpp"
#include "staging.hpp"

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
    // [blobs][blob_off][span_base][qmap][counters], built in a host mirror and uploaded whole (the zeroes of the counters with it)
    StageArena m;
    const auto [s_blobs, s_off, s_span, s_qmap, s_cnt] = std::tuple{m.add<uint8_t>(blob_off[n]), m.add<uint32_t>(n + 1), m.add<uint32_t>(n + 1), m.add<uint32_t>(n), m.add<uint64_t>(counts_off[n])};
    m.commit(ws.d_union_meta);
    std::vector<uint8_t> host(m.whole().n, 0);
    uint8_t* dev = m.dev(s_blobs);
    for (size_t i = 0; i < n; ++i) pack_blob(*cqs[i], idx, host.data() + blob_off[i], dev + blob_off[i], 0, counts_off[i], {}, {});
    std::memcpy(host.data() + s_off.off, blob_off.data(), (n + 1) * 4);
    std::memcpy(host.data() + s_span.off, span_base.data(), (n + 1) * 4);
    std::memcpy(host.data() + s_qmap.off, qmap.data(), n * 4);
    m.upload(m.whole(), host.data(), st);
    {
        uint64_t id_bytes = 0;  // presence only: the doc ids of every list
        for (size_t i = 0; i < n; ++i) id_bytes += 4ull * cqs[i]->total_len;
        LaunchTimer timer(idx.profile.enabled, ws, st, K_COUNT_PREPASS, id_bytes, id_bytes, n);
        launch_tile_scan(st, span_base[n], lds_bytes, dev, m.dev(s_off), m.dev(s_span), m.dev(s_qmap), uint32_t(n), stack_depth, cand_cap, uint32_t(desc_cap), nullptr,
                         reinterpret_cast<unsigned long long*>(m.dev(s_cnt)), nullptr, false, list_table);
    }
    VQ_HIP(hipGetLastError());
    std::vector<uint64_t> cnt(counts_off[n]);
    m.download(s_cnt, cnt.data(), st);
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

// The count pre-pass of the batch's queries that are one (`need`: their positions) -> their numbers, on a sharded index summed over the shards
// (`sum` off: as this shard's kernel wrote them — vq_debug_node_counts)
static std::vector<QueryCounts> measure_counts(const Index& idx, Workspace& ws, PartialBatch& pb, hipStream_t pst, std::vector<size_t>& need, bool sum = true) {
    std::vector<CompiledQuery*> cqs;
    for (size_t i = 0; i < pb.queries.size(); ++i)
        if (pb.queries[i].status == kStatusNeedsCounts) {
            need.push_back(i);
            cqs.push_back(&pb.queries[i]);
        }
    std::vector<QueryCounts> counts;
    if (need.empty()) return counts;
    run_count_queries(idx, ws, cqs, counts, pst);
    if (idx.sharded() && sum) {  // result sizes are sums over the shards
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
    return counts;
}

// ANDs whose summation order / label follow run-time operand sizes: count pre-pass, then the final compilation
static void compile_with_counts(const Index& idx, Workspace& ws, PartialBatch& pb, const vqreq::Request* const* reqs, BatchTables& tables, hipStream_t pst) {
    std::vector<size_t> need;
    const std::vector<QueryCounts> counts = measure_counts(idx, ws, pb, pst, need);
    for (size_t k = 0; k < need.size(); ++k) {
        CompiledQuery& q = pb.queries[need[k]];
        q = compile_query(idx, *reqs[need[k]], tables.later_pass(&counts[k]));
        if (q.status < 0) {
            q.status = ERR_UNSUPPORTED;
            q.error = "unsupported on the MI355X query path: query still needs a pre-pass after the count pre-pass (internal)";
        }
    }
}

// Dictionary scans (fuzzy / prefix leaves) of the whole batch, then its compilation passes up to the count pre-pass, with the job pre-passes
// between them: pb.queries, where a query that IS a count pre-pass still waits for its numbers.  Returns the pre-passes' stream.
static hipStream_t compile_before_counts(const Index& idx, Workspace& ws, PartialBatch& pb, const vqreq::Request* const* reqs, size_t n, hipStream_t st, BatchTables& tables,
                                         CompileReport& rep) {
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
    return pst;
}

// The whole compilation of a batch: the passes above, the count pre-pass and the final compilation of the queries that asked for it
static CompileReport compile_batch(const Index& idx, Workspace& ws, PartialBatch& pb, const vqreq::Request* const* reqs, size_t n, hipStream_t st) {
    CompileReport rep;
    BatchTables tables;
    const hipStream_t pst = compile_before_counts(idx, ws, pb, reqs, n, st, tables, rep);
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

    pb.layout = partial_layout(L.nq, L.total_keys, L.total_hist);
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
    hipStream_t st = pb.scan_stream;
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

std::unique_ptr<PartialBatch> run_partial(const Index& idx, const vqreq::Request* const* reqs, size_t n, int slot, int64_t arena_offset, hipStream_t scan_stream) {
    const double t_start = now_ms();
    auto pb = std::make_unique<PartialBatch>();
    pb->index = &idx;
    pb->reqs.assign(reqs, reqs + n);
    pb->t0 = std::chrono::steady_clock::now();
    pb->scan_stream = scan_stream ? scan_stream : idx.stream;
    acquire_workspace(idx, *pb, slot);
    VQ_HIP(hipSetDevice(idx.device));
    Workspace& ws = *pb->ws;
    ws.timed.clear();
    ws.ev_used = 0;
    pb->profiled = idx.profile.enabled;

    const CompileReport compiled = compile_batch(idx, ws, *pb, reqs, n, pb->scan_stream);
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

// vq_debug_*_lists (capi_debug.cpp): pre-pass drivers alone, on the next workspace in turn (held until `body` returns: the drivers' results live in
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

// A batch's compilation up to the count pre-pass and nothing launched behind it, on a workspace debug_prepass took: where vq_debug_node_counts and
// vq_docset_from_filter start.  Returns the pre-passes' stream.
static hipStream_t compile_without_scan(const Index& idx, Workspace& ws, PartialBatch& pb, const vqreq::Request* const* reqs, size_t n, BatchTables& tables) {
    pb.index = &idx;
    CompileReport rep;
    return compile_before_counts(idx, ws, pb, reqs, n, idx.stream, tables, rep);
}

// vq_debug_node_counts (capi.cpp): a batch's compilation up to and including its count pre-pass — the dictionary scans and job pre-passes its
// leaves need first, run_count_queries on the queries that are one —, and no result scan
std::vector<NodeCounts> debug_node_counts(const Index& idx, const vqreq::Request* const* reqs, size_t n, bool summed) {
    std::vector<NodeCounts> out(n);
    debug_prepass(idx, [&](Workspace& ws, hipStream_t) {
        PartialBatch pb;
        BatchTables tables;
        const hipStream_t pst = compile_without_scan(idx, ws, pb, reqs, n, tables);
        for (size_t i = 0; i < n; ++i) {
            const CompiledQuery& q = pb.queries[i];
            out[i].status = q.status == kStatusNeedsCounts ? 0 : q.status == 0 ? kNodeCountsNone : q.status > 0 ? q.status : int(ERR_UNSUPPORTED);
            if (q.status != 0 && q.status != kStatusNeedsCounts) out[i].error = q.error;
            if (q.status == kStatusNeedsCounts) out[i].n_spans = q.n_spans, out[i].tile_words = q.tile_words;
        }
        std::vector<size_t> need;
        const std::vector<QueryCounts> counts = measure_counts(idx, ws, pb, pst, need, summed);
        for (size_t k = 0; k < need.size(); ++k) {
            NodeCounts& o = out[need[k]];
            o.has_filter = counts[k].has_filter;
            o.filter_count = counts[k].filter_count;
            for (uint32_t node : pb.queries[need[k]].count_nodes) {  // in counter order
                const auto& c = counts[k].nodes.at(node);
                o.nodes.push_back({node, c.first, c.second});
            }
        }
    });
    return out;
}

// vq_docset_from_filter (capi.cpp): the filter compiled alone, as a batch of one compiles it up to the count pre-pass (a filter has no score sums
// to order: there is none) — dictionary scans first, the job pre-passes a leaf asks for —, its lists and program staged in one blob (pack_blob: the
// inline lists travel inside it), then the doc set's image from the program's bits.  The workspace is held until the image is built: a job's
// result lives in it.
std::shared_ptr<const DocSet> make_docset_from_filter(const Index& idx, const vqreq::SearchRequest& filter, std::shared_ptr<const DocSet> within) {
    if (within && within->index_uid != idx.uid) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "the doc set to search within was made for another index");
    if (!idx.can_sum_over_shards())  // the set's length is a sum over the shards
        throw VelociError(ERR_UNSUPPORTED, "unsupported on the MI355X query path: doc set from a filter on a sharded index without vq_index_set_allreduce");
    vqreq::Request req;
    req.filter = filter;
    req.docset = std::move(within);
    req.filter_only = true;
    std::shared_ptr<const DocSet> out;
    debug_prepass(idx, [&](Workspace& ws, hipStream_t) {
        PartialBatch pb;
        BatchTables tables;
        const vqreq::Request* reqs[1] = {&req};
        const hipStream_t pst = compile_without_scan(idx, ws, pb, reqs, 1, tables);
        const CompiledQuery& cq = pb.queries[0];
        if (cq.status > 0) throw VelociError(cq.status, cq.error);
        if (cq.status < 0) throw VelociError(ERR_UNSUPPORTED, "unsupported on the MI355X query path: filter still needs a pre-pass after its jobs ran (internal)");
        // what the kernel relies on: the stack never holds more than stack_depth entries and ends with one, every list exists
        uint32_t sp = 0;
        for (const DOp& op : cq.fops) {
            bool ok = true;
            if (op.kind == OP_LEAF) ok = size_t(op.list_begin) + op.list_count <= cq.lists.size();
            else if ((op.kind == OP_AND || op.kind == OP_OR) && op.nchild >= 1 && op.nchild <= sp) sp -= op.nchild;
            else ok = false;
            if (!ok || ++sp > cq.stack_depth) throw VelociError(ERR_UNSUPPORTED, "unsupported on the MI355X query path: malformed filter program (internal)");
        }
        if (sp != 1 || cq.stack_depth > uint32_t(kStackDepth)) throw VelociError(ERR_UNSUPPORTED, "unsupported on the MI355X query path: malformed filter program (internal)");
        const size_t bytes = pack_blob(cq, idx, nullptr, nullptr, 0, 0, {}, {});
        std::vector<uint8_t> host(bytes);
        DevBuf blob;
        blob.alloc(bytes + 16);
        pack_blob(cq, idx, host.data(), blob.as<uint8_t>(), 0, 0, {}, {});
        blob.upload(host.data(), bytes, pst);
        QHeader h;
        std::memcpy(&h, host.data(), sizeof h);
        out = make_docset_from_program(idx, pst, reinterpret_cast<const DList*>(blob.as<uint8_t>() + h.off_lists), h.n_lists,
                                       reinterpret_cast<const DOp*>(blob.as<uint8_t>() + h.off_fops), h.n_fops, cq.stack_depth);
    });
    return out;
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
        const size_t down_words = ns * 2 + ns * size_t(stride) * 2;
        StageArena meta;
        const auto [s_rows, s_top, s_down] = std::tuple{meta.add<TextRowD>(rows.size()), meta.add<uint32_t>(ns), meta.add<uint32_t>(down_words)};
        meta.commit(d_meta, 16);
        d_best.ensure(ns * size_t(num_texts) * 4 + 16);
        uint32_t* d_counts = meta.dev(s_down);
        meta.upload(s_rows, rows.data(), st);
        meta.upload(s_top, top_ns.data(), st);
        VQ_HIP(hipMemsetAsync(d_best.p, 0, ns * size_t(num_texts) * 4, st));
        {  // layout bytes: the row values read plus 4 B per atomic
            LaunchTimer timer(timed, ws, st, K_TEXT_BEST, values * 8, values * 8, ns);
            launch_text_best(st, meta.dev(s_rows), uint32_t(rows.size()), d_vals, num_texts, d_best.as<uint32_t>());
        }
        {  // num_texts x 4 B per pass over a slot's array: four radix passes, the count of the threshold's equals, the write
            LaunchTimer timer(timed, ws, st, K_TEXT_SELECT, uint64_t(ns) * num_texts * 4 * 6, uint64_t(ns) * num_texts * 4, ns);
            launch_text_select(st, d_best.as<uint32_t>(), num_texts, uint32_t(ns), meta.dev(s_top), stride, d_counts, d_counts + 2 * ns);
        }
        VQ_HIP(hipGetLastError());
        std::vector<uint32_t> down(down_words);
        meta.download(s_down, down.data(), st);
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

// ---- the two merges alone (vq_debug_merge_spans / vq_debug_finalize): one zero-filled QHeader per job with only the fields the kernel reads,
// ONE launch of the shipped launcher over all jobs.  The callers (capi_debug.cpp) have checked the arguments
namespace {
// blobs + blob_off of the jobs' headers -> device; fill(j, header) sets job j's fields beside top_k and part_keys_off (the prefix of top_k)
template <class Fill>
void debug_upload_headers(DevBuf& d_blobs, DevBuf& d_blob_off, const uint32_t* top_k, uint32_t n_jobs, Fill fill) {
    const size_t blob = align_up(sizeof(QHeader), 16);
    std::vector<uint8_t> blobs(n_jobs * blob, 0);
    std::vector<uint32_t> off(n_jobs);
    uint32_t keys = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        QHeader H{};
        H.top_k = top_k[j];
        H.part_keys_off = keys;
        keys += top_k[j];
        fill(j, H);
        off[j] = uint32_t(j * blob);
        std::memcpy(blobs.data() + j * blob, &H, sizeof H);
    }
    d_blobs.alloc(blobs.size());
    d_blobs.upload(blobs.data(), blobs.size());
    d_blob_off.alloc(off.size() * 4);
    d_blob_off.upload(off.data(), off.size() * 4);
}
void debug_download(void* dst, const DevBuf& src, size_t bytes) { VQ_HIP(hipMemcpy(dst, src.p, bytes, hipMemcpyDeviceToHost)); }
}  // namespace

void debug_merge_spans(const uint64_t* span_keys, const uint32_t* n_spans, const uint32_t* top_k, uint32_t n_jobs, uint64_t* out_keys) {
    DevBuf d_blobs, d_blob_off, d_span, d_part;
    size_t in_keys = 0, n_out = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) n_out += top_k[j];
    debug_upload_headers(d_blobs, d_blob_off, top_k, n_jobs, [&](uint32_t j, QHeader& H) {
        H.n_spans = n_spans[j];
        H.keys_base = uint32_t(in_keys);
        in_keys += size_t(n_spans[j]) * top_k[j];
    });
    d_span.alloc(in_keys * 8);
    d_span.upload(span_keys, in_keys * 8);
    d_part.alloc(n_out * 8);
    VQ_HIP(hipMemset(d_part.p, 0xFF, n_out * 8));  // (not zero: a slot the kernel leaves alone shows)
    launch_merge_spans(nullptr, n_jobs, d_blobs.as<uint8_t>(), d_blob_off.as<uint32_t>(), d_span.as<unsigned long long>(), d_part.as<unsigned long long>());
    VQ_HIP(hipDeviceSynchronize());
    debug_download(out_keys, d_part, n_out * 8);
}

void debug_finalize(const uint64_t* shard_keys, const uint64_t* shard_hits, uint32_t num_shards, size_t stride_pad, const uint32_t* top_k, uint32_t n_jobs,
                    uint32_t* out_ids, uint32_t* out_score_bits, uint32_t* out_n, uint64_t* out_hits) {
    DevBuf d_blobs, d_blob_off, d_gathered, d_ids, d_scores, d_n, d_hits;
    size_t keys = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) keys += top_k[j];
    const PartialLayout lay = partial_layout(n_jobs, keys, 0);
    const size_t stride = size_t(lay.off_hist) + stride_pad;
    std::vector<uint8_t> gathered(stride * num_shards, 0);
    for (uint32_t s = 0; s < num_shards; ++s) {
        std::memcpy(gathered.data() + s * stride + lay.off_hits, shard_hits + size_t(s) * n_jobs, size_t(n_jobs) * 8);
        std::memcpy(gathered.data() + s * stride + lay.off_keys, shard_keys + size_t(s) * keys, keys * 8);
    }
    debug_upload_headers(d_blobs, d_blob_off, top_k, n_jobs, [](uint32_t, QHeader&) {});
    d_gathered.alloc(gathered.size());
    d_gathered.upload(gathered.data(), gathered.size());
    const std::pair<DevBuf*, size_t> outs[] = {{&d_ids, keys * 4}, {&d_scores, keys * 4}, {&d_n, size_t(n_jobs) * 4}, {&d_hits, size_t(n_jobs) * 8}};
    for (const auto& o : outs) {
        o.first->alloc(o.second);
        VQ_HIP(hipMemset(o.first->p, 0xFF, o.second));
    }
    launch_finalize(nullptr, n_jobs, d_blobs.as<uint8_t>(), d_blob_off.as<uint32_t>(), d_gathered.as<uint8_t>(), num_shards, stride, lay, d_ids.as<uint32_t>(),
                    d_scores.as<float>(), d_n.as<uint32_t>(), d_hits.as<unsigned long long>());
    VQ_HIP(hipDeviceSynchronize());
    debug_download(out_ids, d_ids, keys * 4);
    debug_download(out_score_bits, d_scores, keys * 4);
    debug_download(out_n, d_n, size_t(n_jobs) * 4);
    debug_download(out_hits, d_hits, size_t(n_jobs) * 8);
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
    if (st != pb.scan_stream) VQ_HIP(hipStreamWaitEvent(st, ws.ev_done, 0));
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
        // top_n_sort (sort.rs:5-22) starts from worst_score = f32::MIN and passes over every hit below it: a hit whose score is -inf (a Log boost
        // of a column value 0) counts in num_hits and is never returned.  Such hits rank last: they are the tail of the ranked window
        uint32_t returnable = have;
        while (returnable && scores[returnable - 1] < -std::numeric_limits<float>::max()) --returnable;
        // apply_top_skip (search.rs:230-239) on the top+skip window
        const uint32_t want = cq.top + cq.skip;
        const uint32_t avail = std::min(returnable, want);
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
