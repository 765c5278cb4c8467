// Pre-pass runners: the device work a batch does before its scan, whose results the compiler consumes (dictionary scans and the leaf top-n,
// materialised unions, range counts, text-locality and 1:n boost lists).  compile_batch (exec.cpp) calls them between its compilation passes.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "staging.hpp"

#include "text.hpp"

namespace vq {

using namespace vqreq;

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
    // tables: [rank_of][descriptors][class ord] up, [seg: 2 * n_ranks + 1][out_off: n_topn + 1][out_n: n_topn] down (one table: one copy back)
    const size_t seg_words = 2 * size_t(n_ranks) + 1, down_words = seg_words + 2 * size_t(n_topn) + 1;
    StageArena meta;
    const auto [s_rank, s_desc, s_ord, s_down] = std::tuple{meta.add<uint32_t>(n_ranks), meta.add<TopnProbeD>(descs.size()), meta.add<uint16_t>(kTopnClasses), meta.add<uint32_t>(down_words)};
    meta.commit(ws.d_topn_meta, 16);
    uint32_t* d_seg = meta.dev(s_down);
    StageArena sorted;
    const auto [s_keys, s_keys_sorted, s_infos, s_infos_sorted] = std::tuple{sorted.add<unsigned long long>(count), sorted.add<unsigned long long>(count), sorted.add<uint32_t>(count), sorted.add<uint32_t>(count)};
    sorted.commit(ws.d_topn_sort, 16);
    const size_t tmp_bytes = dict_topn_sort_tmp_bytes(count, n_ranks);
    if (tmp_bytes == size_t(-1)) throw VelociError(ERR_DEVICE, "leaf top-n: the grouping sort's storage size");
    ws.d_topn_tmp.ensure(tmp_bytes + 16);
    ws.d_topn_out.ensure(size_t(std::min<uint64_t>(room, count)) * 8 + 16);  // (the buffers are packed: a probe gets min(its matches, top_n + 200) entries)
    meta.upload(s_rank, rank_of.data(), st);
    meta.upload(s_desc, descs.data(), st);
    meta.upload(s_ord, classes.ord, st);
    {
        LaunchTimer timer(idx.profile.enabled, ws, st, K_DICT_TOPN_GROUP, uint64_t(count) * (12 + 2 * 12), uint64_t(count) * 12, n_ranks);
        if (!launch_dict_topn_group(st, d_recs, count, meta.dev(s_rank), n_ranks, n_full, sorted.dev(s_keys), sorted.dev(s_keys_sorted), sorted.dev(s_infos),
                                    sorted.dev(s_infos_sorted), ws.d_topn_tmp.p, tmp_bytes, d_seg))
            throw VelociError(ERR_DEVICE, "leaf top-n: the grouping sort could not be queued");
    }
    {
        LaunchTimer timer(idx.profile.enabled, ws, st, K_DICT_TOPN, 0, 0, n_topn);
        launch_dict_topn(st, meta.dev(s_desc), n_topn, max_top_n, sorted.dev(s_keys_sorted), sorted.dev(s_infos_sorted), d_seg, meta.dev(s_ord), d_seg + seg_words,
                         d_seg + seg_words + n_topn + 1, ws.d_topn_out.as<unsigned long long>());
    }
    VQ_HIP(hipGetLastError());
    std::vector<uint32_t> down(down_words);
    meta.download(s_down, down.data(), st);
    VQ_HIP(hipStreamSynchronize(st));
    const uint32_t full_records = down[seg_words - 1];
    const uint32_t* out_off = down.data() + seg_words;
    const uint32_t* out_n = out_off + n_topn + 1;
    if (full_records > count || out_off[n_topn] > count - full_records) throw VelociError(ERR_DEVICE, "leaf top-n: more records to copy back than there are");
    std::vector<unsigned long long> bufs(out_off[n_topn]), keys(full_records);
    std::vector<uint32_t> infos(full_records);
    if (!bufs.empty()) VQ_HIP(hipMemcpyAsync(bufs.data(), ws.d_topn_out.p, bufs.size() * 8, hipMemcpyDeviceToHost, st));
    sorted.download(s_keys_sorted.sub(0, full_records), keys.data(), st);  // (the full-route probes' records: the front of the sorted arrays)
    sorted.download(s_infos_sorted.sub(0, full_records), infos.data(), st);
    VQ_HIP(hipStreamSynchronize(st));
    recs.resize(full_records);
    for (uint32_t r = 0; r < full_records; ++r) {
        const uint32_t rank = uint32_t(keys[r] >> 32);
        if (rank >= n_full) throw VelociError(ERR_DEVICE, "leaf top-n: a top-n probe's record inside the full-route piece");
        recs[r] = DictMatch{probe_of[rank], uint32_t(keys[r]), infos[r]};
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
void topn_class_ords(uint16_t* ord) { std::memcpy(ord, topn_classes().ord, sizeof topn_classes().ord); }

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
    DevBuf &d_count = ws.d_probe_counts, &d_out = ws.d_probe_ids;
    // one descriptor buffer: [DictProbe x N][DictProbeW x N][pool]
    StageArena desc;
    const auto [s_probes, s_wprobes, s_pool] = std::tuple{desc.add<DictProbe>(probes.size()), desc.add<DictProbeW>(wprobes.size()), desc.add<uint32_t>(pool.size())};
    desc.commit(ws.d_probe_desc, 16);
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
    StageArena regex;
    const auto [s_rprobes, s_rpool] = std::tuple{regex.add<RegexProbeD>(rprobes.size()), regex.add<uint16_t>(rpool.size())};
    if (!rprobes.empty()) {
        regex.commit(ws.d_regex_tabs, 16);
        regex.upload(s_rprobes, rprobes.data(), st);
        regex.upload(s_rpool, rpool.data(), st);
    }
    desc.upload(s_probes, probes.data(), st);
    desc.upload(s_wprobes, wprobes.data(), st);
    desc.upload(s_pool, pool.data(), st);  // (filled by the pooled probes only)
    uint32_t cap = uint32_t(std::max<size_t>(64 * todo.size(), 1u << 16));  // matches of the whole batch share one output array
    std::vector<DictMatch> recs;
    uint64_t scan_bytes = 0, regex_bytes = 0;  // every probe reads its dictionary once (offsets + code points) ...
    for (size_t i = 0; i < todo.size(); ++i) {
        const Dictionary& d = idx.dict.at(todo[i]->path);
        (i < n_scan ? scan_bytes : regex_bytes) += d.d_off.bytes + (i < n_scan ? d.d_low : d.d_raw).bytes;
    }
    for (int pass = 0; pass < 2; ++pass) {  // pass 1 only when the matches outgrew the first guess (the count is exact then)
        d_out.ensure(size_t(cap) * sizeof(DictMatch) + 16);
        VQ_HIP(hipMemsetAsync(d_count.p, 0, 4, st));
        if (n_scan) {
            uint64_t layout = 0;
            LaunchTimer timer(idx.profile.enabled, ws, st, K_DICT_SCAN, 0, scan_bytes, n_scan);
            for (size_t g0 = 0; g0 < n_scan;) {  // one launch per run of probes over the same image
                size_t g1 = g0 + 1;
                while (g1 < n_scan && image_of(*todo[g1]) == image_of(*todo[g0]) && is_pooled[g1] == is_pooled[g0]) ++g1;
                const Dictionary& d = idx.dict.at(todo[g0]->path);
                if (is_pooled[g0])
                    launch_dict_scan_wide(st, d.char_bytes, desc.dev(s_wprobes) + g0, desc.dev(s_pool), uint32_t(g0), uint32_t(g1 - g0), d.d_off.as<uint32_t>(),
                                          image_of(*todo[g0]), d.d_low.p, uint32_t(d.terms.size()), d_count.as<uint32_t>(), cap, d_out.as<DictMatch>());
                else
                    launch_dict_scan(st, desc.dev(s_probes) + g0, uint32_t(g0), uint32_t(g1 - g0), d.d_off.as<uint32_t>(),
                                     static_cast<const uint16_t*>(image_of(*todo[g0])), d.d_low.as<uint16_t>(), uint32_t(d.terms.size()), d_count.as<uint32_t>(), cap,
                                     d_out.as<DictMatch>());
                layout += (d.d_off.bytes + d.d_low.bytes) * ((g1 - g0 + 15) / 16);  // ... this layout: once per 16 probes of one image
                g0 = g1;
            }
            if (!ws.timed.empty() && idx.profile.enabled) ws.timed.back().layout_bytes = layout;
        }
        if (n_scan < todo.size()) {  // k_dict_regex: grid.y = probe, every probe reads its dictionary's offsets and raw image (and its own tables)
            LaunchTimer timer(idx.profile.enabled, ws, st, K_DICT_REGEX, regex_bytes + rpool.size() * 2, regex_bytes, todo.size() - n_scan);
            for (size_t g0 = n_scan; g0 < todo.size();) {  // one launch per run of probes over one dictionary with tables of one size class
                size_t g1 = g0 + 1;
                const bool small = small_tables(*todo[g0]);
                while (g1 < todo.size() && image_of(*todo[g1]) == image_of(*todo[g0]) && small_tables(*todo[g1]) == small) ++g1;
                const Dictionary& d = idx.dict.at(todo[g0]->path);
                launch_dict_regex(st, d.char_bytes, small, regex.dev(s_rprobes) + (g0 - n_scan), regex.dev(s_rpool), d.d_alpha.as<uint32_t>(),
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
        if (timing_enabled()) std::fprintf(stderr, "[vq timing] dictionary scan: %zu probes, %u matches\n", todo.size(), count);
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
    if (timing_enabled()) {  // the distribution of matches over the probes (a few short probes can hold most of them)
        std::vector<uint32_t> per(todo.size(), 0);
        for (auto& r : recs) per[r.probe]++;
        std::sort(per.begin(), per.end(), std::greater<uint32_t>());
        std::string top;
        for (size_t i = 0; i < per.size() && i < 8; ++i) top += " " + std::to_string(per[i]);
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
    StageArena m;
    const auto s_lists = m.add<UList>(ulists.size());
    const auto s_tasks = m.add<UTask>(utasks.size());
    const auto s_span_task = m.add<uint32_t>(n_spans), s_cnt = m.add<uint32_t>(n_spans);
    const auto s_off = m.add<uint64_t>(n_spans);
    m.commit(meta);
    m.upload(s_lists, ulists.data(), st);
    m.upload(s_tasks, utasks.data(), st);
    m.upload(s_span_task, span_task.data(), st);
    uint64_t in_bytes = 0;
    for (auto& u : ulists) in_bytes += uint64_t(u.len) * ((u.flags & 1u) ? 8u : 6u);
    uint64_t out_bytes = 0;
    auto launch = [&](bool write) {
        LaunchTimer timer(timed, ws, st, write ? K_UNION_WRITE : K_UNION_COUNT, in_bytes + (write ? out_bytes : 0), in_bytes + (write ? out_bytes : 0), tasks.size());
        launch_union(st, write, uint32_t(n_spans), m.dev(s_lists), m.dev(s_tasks), m.dev(s_span_task), m.dev(s_cnt), m.dev(s_off), docs.as<uint32_t>(), vals.as<float>(),
                     maxes.as<uint32_t>());
        VQ_HIP(hipGetLastError());
    };
    launch(false);
    std::vector<uint32_t> cnt(n_spans);
    m.download(s_cnt, cnt.data(), st);
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
        cursor += padded_list_len(len);
    }
    out_bytes = cursor * 8;
    docs.ensure(cursor * 4 + 64);
    vals.ensure(cursor * 4 + 64);
    maxes.ensure(tasks.size() * 4 + 64);
    VQ_HIP(hipMemsetAsync(maxes.p, 0xFF, tasks.size() * 4, st));  // min(~order(value)) per task, written by the write pass
    m.upload(s_off, off.data(), st);
    launch(true);
    // the largest value of every merged list: the compiler's score bounds need it (top-k pruning of the scan)
    std::vector<uint32_t> mins(tasks.size());
    VQ_HIP(hipMemcpyAsync(mins.data(), maxes.p, tasks.size() * 4, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    for (size_t t = 0; t < tasks.size(); ++t) {
        UnionTaskH& T = tasks[t];
        if (!T.job) continue;  // (a level-1 piece of a wider job: run_union_jobs hands it to level 2)
        T.job->d_docs = docs.as<uint32_t>() + T.out_off;
        T.job->d_vals = vals.as<float>() + T.out_off;
        T.job->max_value = mins[t] != 0xFFFFFFFFu ? value_of_order_key(~mins[t]) : 0.0f;
        T.job->len = T.len;
    }
}

// K2 for wide leaves (union_dense.hip): a u32 key per doc of the shard's range in a slab, raised by one atomic max per posting, then compacted
// into k_union<write>'s output format.  The jobs run in groups whose slabs fit the budget; nothing comes back to the host between the
// launches, the lengths and largest values of all jobs are fetched in one read-back at the end.  A job's output slice is sized by its upper
// bound, min(postings, docs of the range).
long long env_clamped(const char* name, long long unset, long long lo, long long hi) {
    const char* e = std::getenv(name);
    return std::min(std::max(e ? std::atoll(e) : unset, lo), hi);
}
size_t union_dense_min() {  // jobs with more lists than this take the dense route (two levels of k_union take no more than 64 x 64)
    static const size_t v = size_t(env_clamped("VQ_UNION_DENSE_MIN", 64 * 64, 1, 64 * 64));
    return v;
}
uint64_t union_dense_slab_budget() {  // bytes of slabs alive at once (a job always gets one)
    static const uint64_t v = uint64_t(env_clamped("VQ_UNION_DENSE_SLAB_MB", 1024, 0, 1ll << 20)) << 20;
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
            out_cursor += padded_list_len(cap[jb + k]);
        }
        g.n_lists = lists.size() - g.list_begin;
        if (g.n_lists > 0xFFFFFFF0ull) throw VelociError(ERR_UNSUPPORTED, "leaf expansions of one batch with more than 2^32 posting lists");
        UDenseList end{};
        end.first = g.postings;
        lists.push_back(end);
        groups.push_back(g);
    }
    StageArena m;
    const auto [s_lists, s_jobs, s_res, s_cnt, s_max] = std::tuple{m.add<UDenseList>(lists.size()), m.add<UDenseJob>(djobs.size()), m.add<UDenseResult>(jobs.size()),
                                                                   m.add<uint32_t>(per_group * size_t(job_blocks)), m.add<uint32_t>(per_group * size_t(job_blocks))};
    m.commit(ws.d_union_dense_meta);
    ws.d_union_slab.ensure(per_group * slab_words * 4);
    ws.d_union_dense_docs.ensure(out_cursor * 4 + 64);
    ws.d_union_dense_vals.ensure(out_cursor * 4 + 64);
    uint32_t* slab = ws.d_union_slab.as<uint32_t>();
    m.upload(s_lists, lists.data(), st);
    m.upload(s_jobs, djobs.data(), st);
    m.zero(s_res, st);  // (a group without postings launches no scatter; its lists are empty all the same)
    const bool timed = idx.profile.enabled;
    std::vector<std::pair<size_t, size_t>> write_slots;  // (timed launch, group): the write pass's output bytes are known after the read-back
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const Group& g = groups[gi];
        const uint32_t n_blocks = uint32_t(g.n_jobs) * job_blocks;
        const uint64_t slab_bytes = g.n_jobs * slab_words * 4;
        {  // slab clear + scatter: 4 B per doc written, 6 B per posting read, one 4-byte atomic per posting
            LaunchTimer timer(timed, ws, st, K_UNION_DENSE_SCATTER, slab_bytes + g.postings * 10, g.postings * 6, g.n_jobs);
            VQ_HIP(hipMemsetAsync(slab, 0, slab_bytes, st));
            launch_union_dense_scatter(st, m.dev(s_lists) + g.list_begin, uint32_t(g.n_lists), g.postings, m.dev(s_jobs) + g.job_begin, slab, idx.doc_lo, range);
            VQ_HIP(hipGetLastError());
        }
        {  // 4 B per doc read; a count and a largest key per block written, read again by the prefix sums, the offsets written
            LaunchTimer timer(timed, ws, st, K_UNION_DENSE_COUNT, slab_bytes + uint64_t(n_blocks) * 20, slab_bytes, g.n_jobs);
            launch_union_dense_count(st, m.dev(s_jobs) + g.job_begin, uint32_t(g.n_jobs), n_blocks, slab, m.dev(s_cnt), m.dev(s_max), m.dev(s_res));
            VQ_HIP(hipGetLastError());
        }
        {  // 4 B per doc read, 8 B per entry written (added below)
            LaunchTimer timer(timed, ws, st, K_UNION_DENSE_WRITE, slab_bytes + uint64_t(n_blocks) * 4, slab_bytes, g.n_jobs);
            if (timer.ws) write_slots.push_back({timer.slot, gi});
            launch_union_dense_write(st, m.dev(s_jobs) + g.job_begin, uint32_t(g.n_jobs), n_blocks, slab, m.dev(s_cnt), idx.doc_lo, ws.d_union_dense_docs.as<uint32_t>(),
                                     ws.d_union_dense_vals.as<float>());
            VQ_HIP(hipGetLastError());
        }
    }
    std::vector<UDenseResult> res(jobs.size());
    m.download(s_res, res.data(), st);
    VQ_HIP(hipStreamSynchronize(st));
    for (size_t j = 0; j < jobs.size(); ++j) {
        if (res[j].len > cap[j]) throw VelociError(ERR_DEVICE, "dense union wrote more entries than its postings (internal)");
        if (res[j].len > 0xFFFFFFF0u) throw VelociError(ERR_UNSUPPORTED, "materialised leaf longer than 2^32 entries");
        UnionJob& job = *jobs[j];
        job.d_docs = ws.d_union_dense_docs.as<uint32_t>() + djobs[j].out_off;
        job.d_vals = ws.d_union_dense_vals.as<float>() + djobs[j].out_off;
        job.len = res[j].len;
        job.max_value = res[j].max_key ? value_of_order_key(res[j].max_key) : 0.0f;
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
        if (raw.size() <= 64) l1.push_back(UnionTaskH{std::move(raw), &job});
        else {
            for (size_t b = 0; b < raw.size(); b += 64)
                l1.push_back(UnionTaskH{std::vector<UList>(raw.begin() + b, raw.begin() + std::min(raw.size(), b + 64)), nullptr, l2.size()});
            l2.push_back(UnionTaskH{{}, &job});
        }
    }
    run_union_dense(idx, ws, dense, st);
    run_union_level(idx.profile.enabled, ws, l1, ws.d_union_docs[0], ws.d_union_vals[0], ws.d_union_max, ws.d_union_meta, st);
    for (auto& t : l1) {  // (the tasks that are a job's whole result have been handed to it)
        if (t.job) continue;
        UList u{};
        u.docs = ws.d_union_docs[0].as<uint32_t>() + t.out_off;
        u.scores = ws.d_union_vals[0].as<float>() + t.out_off;
        u.len = t.len;
        u.term_score = 1.0f;
        u.flags = 1u;
        l2[t.parent].lists.push_back(u);
    }
    run_union_level(idx.profile.enabled, ws, l2, ws.d_union_docs[1], ws.d_union_vals[1], ws.d_union_max, ws.d_union_meta, st);  // (level 1 has synchronised)
}

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
        RangeJobD d{};
        d.list_begin = uint32_t(ulists.size());
        auto add_list = [&](const uint32_t* docs, uint32_t len) {  // (doc ids only: the kernel counts presence)
            UList u{};
            u.docs = docs;
            u.len = len;
            if (len) ulists.push_back(u);
        };
        auto uit = job.union_key.empty() ? unions.end() : unions.find(job.union_key);
        if (uit != unions.end()) add_list(uit->second.d_docs, uit->second.len);  // the leaf was materialised: its merged list holds exactly the leaf's hits
        else
            for (uint32_t tid : job.tokens)
                if (tid < ps.len.size()) add_list(ps.docs.as<uint32_t>() + ps.start[tid], ps.len[tid]);
        d.n_lists = uint32_t(ulists.size()) - d.list_begin;
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
        StageArena m;
        const auto [s_lists, s_jobs, s_anchors, s_cnt] = std::tuple{m.add<UList>(ulists.size()), m.add<RangeJobD>(jobs.size()), m.add<uint32_t>(anchors.size()), m.add<uint64_t>(counts.size())};
        m.commit(ws.d_union_meta);
        m.upload(s_lists, ulists.data(), st);
        m.upload(s_jobs, jobs.data(), st);
        m.upload(s_anchors, anchors.data(), st);
        m.zero(s_cnt, st);
        {
            LaunchTimer timer(idx.profile.enabled, ws, st, K_RANGE_HITS, 0, 0, jobs.size());
            launch_range_hits(st, n_blocks, uint32_t(jobs.size()), m.dev(s_lists), m.dev(s_jobs), m.dev(s_anchors), reinterpret_cast<unsigned long long*>(m.dev(s_cnt)));
        }
        VQ_HIP(hipGetLastError());
        m.download(s_cnt, counts.data(), st);
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

// K7: text locality of fields whose text ids are not anchors, for every (request, field) job of the batch (see kernels.hip, k_loc_*).
void run_locality_jobs(const Index& idx, Workspace& ws, LocalityTable& table, hipStream_t st) {
    std::vector<LocalityJob*> jobs;
    for (auto& kv : table) jobs.push_back(&kv.second);
    if (jobs.empty()) return;
    // all jobs of one table next to each other: one gather launch per tokens_to_text_id table
    std::stable_sort(jobs.begin(), jobs.end(), [](const LocalityJob* a, const LocalityJob* b) { return a->t2t_path < b->t2t_path; });
    const size_t nj = jobs.size();
    std::vector<LocJob> dj(nj);
    GatherStage gather;
    for (size_t j = 0; j < nj; ++j) {
        const KVStore& t2a = idx.kv.at(jobs[j]->t2a_path);
        LocJob& J = dj[j];
        std::memset(&J, 0, sizeof J);
        J.t2a_vals = t2a.values.as<uint32_t>();
        J.t2a_start = t2a.d_row_start.as<uint64_t>();
        J.t2a_len = t2a.d_row_len.as<uint32_t>();
        J.t2a_key_base = t2a.key_base;
        J.t2a_num_keys = t2a.num_keys;
        gather.add_job(idx.kv.at(jobs[j]->t2t_path), j == 0 || jobs[j]->t2t_path != jobs[j - 1]->t2t_path, jobs[j]->tokens,
                       "text_locality: more than 2^32 token->text entries in one batch");
        J.seg_begin = gather.seg_begin[j];
        J.seg_end = gather.seg_end[j];
        jobs[j]->d_docs = nullptr;  // (without any entry nothing is launched and the lists stay so)
        jobs[j]->d_vals = nullptr;
        jobs[j]->len = 0;
    }
    const uint32_t E = uint32_t(gather.cursor);
    if (!E) return;
    // meta: [jobs][rows][seg_begin u32][seg_end u32][counters u32][pair_begin u32][pair_end u32][out_len u32]
    StageArena m;
    const auto s_jobs = m.add<LocJob>(nj);
    gather.layout(m);
    const auto s_cnt = m.add<uint32_t>(nj), s_pb = m.add<uint32_t>(nj), s_pe = m.add<uint32_t>(nj), s_len = m.add<uint32_t>(nj);
    m.commit(ws.d_loc_meta);
    ws.d_loc_a.ensure(size_t(E) * 4 + 16);
    ws.d_loc_b.ensure(size_t(E) * 4 + 16);
    LaunchTimer timer(idx.profile.enabled, ws, st, K_LOCALITY, size_t(E) * 16, size_t(E) * 4, nj);
    m.upload(s_jobs, dj.data(), st);
    gather.upload(m, st);
    m.zero(s_cnt, st);
    gather.run(m, ws.d_loc_a, ws.d_loc_b, ws.d_loc_tmp, st);
    // count pass: (anchor, boost) pairs per job
    launch_loc_expand(st, false, m.dev(s_jobs), uint32_t(nj), ws.d_loc_b.as<uint32_t>(), E, m.dev(s_cnt), nullptr);
    VQ_HIP(hipGetLastError());
    std::vector<uint32_t> totals(nj);
    m.download(s_cnt, totals.data(), st);
    VQ_HIP(hipStreamSynchronize(st));
    uint64_t P = 0, out_cursor = 0;
    std::vector<uint32_t> pb(nj), pe(nj);
    for (size_t j = 0; j < nj; ++j) {
        dj[j].pair_begin = pb[j] = uint32_t(P);
        P += totals[j];
        if (P > 0xFFFFFFF0ull) throw VelociError(ERR_UNSUPPORTED, "text_locality: more than 2^32 (anchor, boost) pairs in one batch");
        dj[j].pair_end = pe[j] = uint32_t(P);
        dj[j].out_off = uint32_t(out_cursor);
        out_cursor += padded_list_len(totals[j]);
    }
    ws.d_loc_docs.ensure(out_cursor * 4 + 64);
    ws.d_loc_vals.ensure(out_cursor * 4 + 64);
    m.upload(s_jobs, dj.data(), st);
    if (P) {
        ws.d_loc_pairs_a.ensure(P * 8 + 16);
        ws.d_loc_pairs_b.ensure(P * 8 + 16);
        m.upload(s_pb, pb.data(), st);
        m.upload(s_pe, pe.data(), st);
        m.zero(s_cnt, st);
        launch_loc_expand(st, true, m.dev(s_jobs), uint32_t(nj), ws.d_loc_b.as<uint32_t>(), E, m.dev(s_cnt), ws.d_loc_pairs_a.as<unsigned long long>());
        VQ_HIP(hipGetLastError());
        seg_sort(ws.d_loc_tmp, ws.d_loc_pairs_a.as<unsigned long long>(), ws.d_loc_pairs_b.as<unsigned long long>(), uint32_t(P), uint32_t(nj), m.dev(s_pb), m.dev(s_pe), st);
    }
    launch_loc_compact(st, m.dev(s_jobs), uint32_t(nj), ws.d_loc_pairs_b.as<unsigned long long>(), ws.d_loc_docs.as<uint32_t>(), ws.d_loc_vals.as<float>(), m.dev(s_len));
    VQ_HIP(hipGetLastError());
    std::vector<uint32_t> lens(nj);
    m.download(s_len, lens.data(), st);
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
    GatherStage gather;
    uint64_t out_cursor = 0;
    for (size_t j = 0; j < nj; ++j) {
        const KVStore& to_anchor = idx.kv.at(jobs[j]->to_anchor_path);
        const BoostColumn& col = idx.boost.at(jobs[j]->boost_path);
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
        gather.add_job(idx.kv.at(jobs[j]->to_parent_path), j == 0 || jobs[j]->to_parent_path != jobs[j - 1]->to_parent_path, jobs[j]->text_ids,
                       "1:n field boost: more than 2^32 value ids in one batch");
        J.seg_begin = gather.seg_begin[j];
        J.seg_end = gather.seg_end[j];
        J.out_off = uint32_t(out_cursor);
        out_cursor += padded_list_len(J.seg_end - J.seg_begin);
        if (out_cursor > 0xFFFFFFF0ull) throw VelociError(ERR_UNSUPPORTED, "1:n field boost: more than 2^32 value ids in one batch");
    }
    const uint32_t E = uint32_t(gather.cursor);
    StageArena m;
    const auto s_jobs = m.add<B1nJob>(nj);
    gather.layout(m);
    const auto s_res = m.add<B1nResult>(nj);
    m.commit(ws.d_b1n_meta);
    ws.d_b1n_a.ensure(size_t(E) * 4 + 16);
    ws.d_b1n_b.ensure(size_t(E) * 4 + 16);
    ws.d_b1n_docs.ensure(out_cursor * 4 + 64);
    ws.d_b1n_vals.ensure(out_cursor * 4 + 64);
    const double t_rows = now_ms();
    LaunchTimer timer(idx.profile.enabled, ws, st, K_BOOST1N, size_t(E) * 24, size_t(E) * 12, nj);
    m.upload(s_jobs, dj.data(), st);
    gather.upload(m, st);
    gather.run(m, ws.d_b1n_a, ws.d_b1n_b, ws.d_b1n_tmp, st);  // (no value id at all: nothing to gather, k_b1n_map still writes the empty lists)
    double t_sorted = 0;
    if (timing_enabled()) {
        VQ_HIP(hipStreamSynchronize(st));
        t_sorted = now_ms();
    }
    launch_b1n_map(st, m.dev(s_jobs), uint32_t(nj), ws.d_b1n_b.as<uint32_t>(), ws.d_b1n_docs.as<uint32_t>(), ws.d_b1n_vals.as<float>(), m.dev(s_res));
    VQ_HIP(hipGetLastError());
    std::vector<B1nResult> res(nj);
    m.download(s_res, res.data(), st);
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
                     nj, E, longest, n_several, gather.rows.size(), t_rows - t_begin, t_sorted - t_rows, now_ms() - t_sorted);
    }
}

}  // namespace vq
