// The vq_debug_* hooks that drive one kernel or one pre-pass alone (tests, tools): exported, part of the ABI only where include/veloci_amd.h says so.
// The one-line getters stay beside their families in capi.cpp.
#include <cstdio>
#include <cstring>

#include "capi_internal.hpp"
#include "term_lookup.hpp"

using namespace vq;

#ifndef __HIPCC__
// A host build of this file (the stubbed device layer, csrc/Makefile `asan` / `hoststub`) has no kernels.hip behind vq_debug_col_boost.  Its
// launcher comes from the stub files of the tests tree (tests/native/hip_stub_col_boost.cpp); a tree of stubs from before the hook has none,
// and the host build must still link: this weak definition declines like a stub, and any other definition takes its place.
namespace vq {
__attribute__((weak)) int debug_col_boost(DColBoost, const float*, uint32_t, const uint32_t*, uint32_t, const uint32_t*, const float*, uint32_t, float*, float*) { return -1; }
}  // namespace vq
#endif

// ---- helpers of the vq_debug_*_lists functions below
namespace {
std::string debug_job_key(uint32_t j) {  // the job tables are ordered by key: keys in job order
    char buf[16];
    std::snprintf(buf, sizeof buf, "%010u", j);
    return buf;
}
bool debug_csr_ok(const uint64_t* off, const uint32_t* ids, uint32_t n_jobs) {
    if (!off || off[0] != 0) return false;
    for (uint32_t j = 0; j < n_jobs; ++j)
        if (off[j + 1] < off[j]) return false;
    return off[n_jobs] <= (uint64_t(1) << 31) && (ids || !off[n_jobs]);
}
// the lists of the jobs, back to back: job j's len[j] + 8 entries start at the sum of len[i] + 8 over i < j.  False when out_cap is too small.
// A job without a list on the device (the driver launched nothing for the whole call) leaves its 8 entries as they are.
template <class Job>
bool debug_copy_lists(const std::vector<const Job*>& jobs, uint64_t out_cap, uint32_t* out_docs, uint32_t* out_val_bits) {
    uint64_t need = 0;
    for (const Job* j : jobs) need += uint64_t(j->len) + 8;
    if (need > out_cap) return false;
    uint64_t at = 0;
    for (const Job* j : jobs) {
        if (j->d_docs && j->d_vals) {
            VQ_HIP(hipMemcpy(out_docs + at, j->d_docs, (size_t(j->len) + 8) * 4, hipMemcpyDeviceToHost));
            VQ_HIP(hipMemcpy(out_val_bits + at, j->d_vals, (size_t(j->len) + 8) * 4, hipMemcpyDeviceToHost));
        }
        at += uint64_t(j->len) + 8;
    }
    return true;
}
template <class F>
int debug_run(const vq_index* index, F body) {  // body returns false for an output area that is too small
    try {
        bool fits = true;
        vq::debug_prepass(*index->idx, [&](Workspace& ws, hipStream_t st) { fits = body(ws, st); });
        g_err.clear();
        return fits ? 0 : -2;
    } catch (const std::exception& e) {
        g_err = e.what();  // (vq_last_error says why)
        return -1;
    }
}
}  // namespace

extern "C" {

/* tests (like the accessor above: exported, not part of the header): list `token` of a posting store as the probe kernels' 16-bit array image —
   per 32768-doc tile its entries, in-tile offset << 1 | low score class, padded to a multiple of 8 with 0xFFFF — and the list's raw f16 pivot and
   maximum (pivot == maximum: the list has no class).  -> entries of the image (`out` takes up to `cap` of them); 0: the list has no such image */
uint64_t vq_debug_arr16_list(const vq_index* index, const char* store_path, uint32_t token, uint16_t* out, uint64_t cap, uint16_t* pivot_raw, uint16_t* max_raw) {
    if (!index || !store_path) return 0;
    auto it = index->idx->postings.find(store_path);
    if (it == index->idx->postings.end()) return 0;
    const PostingStore& ps = it->second;
    if (token >= ps.num_tokens || ps.ak_start.empty() || ps.ak_start[token] < 0) return 0;
    const uint64_t ptiles = (index->idx->bitmap_words >> (kProbeTileShift - 5)) + 2;  // (the list's directory ends with the granules below that tile: all of them)
    uint32_t gran = 0;
    if (hipMemcpy(&gran, ps.gdir.as<uint32_t>() + ps.gd_start[token] + ptiles, 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    const uint64_t n = uint64_t(gran) * 8, take = std::min(n, cap);
    if (take && out && hipMemcpy(out, ps.arr16.as<uint16_t>() + uint64_t(ps.ak_start[token]) * 8, take * 2, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (pivot_raw) *pivot_raw = ps.pivot_raw[token];
    if (max_raw) *max_raw = ps.max_raw[token];
    return n;
}
/* self-check (tests): k_dict_topn on one crafted stream of (term, class) in id order -> its final buffer in buffer order (out_terms / out_classes
   take top_n + 200 entries).  0; -1 without a device; -2 for arguments the kernel does not take */
int vq_debug_dict_topn(const uint32_t* terms, const uint32_t* classes, uint32_t n, uint32_t top_n, uint32_t* out_terms, uint32_t* out_classes, uint32_t* out_n) {
    if ((n && (!terms || !classes)) || !out_terms || !out_classes || !out_n || top_n == 0 || top_n > vq::kTopnMax) return -2;
    for (uint32_t i = 0; i < n; ++i)
        if (classes[i] >= vq::kTopnClasses) return -2;
    uint16_t ord[vq::kTopnClasses];
    vq::topn_class_ords(ord);
    return vq::debug_dict_topn(terms, classes, n, top_n, ord, out_terms, out_classes, out_n);
}
/* self-check (tests): k_text_best + k_text_select on a caller's CSR -> the top_n texts by (score bits descending, text id ascending) and the number
   of touched texts.  0; -1 without a device; -2 for arguments the kernels do not take */
int vq_debug_text_rank(const uint64_t* row_off, const uint32_t* row_vals, const uint32_t* row_score_bits, uint32_t num_rows, uint32_t num_texts, uint32_t top_n,
                       uint32_t* out_texts, uint32_t* out_score_bits, uint32_t* out_n, uint32_t* out_touched) {
    if (!row_off || (num_rows && !row_score_bits) || !out_texts || !out_score_bits || !out_n || !out_touched) return -2;
    if (top_n == 0 || top_n > vq::kTextRankMaxTop || num_texts == 0 || uint64_t(num_texts) * 4 > vq::kTextRankBudget || row_off[0] != 0) return -2;
    for (uint32_t r = 0; r < num_rows; ++r) {
        if (row_off[r + 1] < row_off[r] || row_score_bits[r] == 0 || row_score_bits[r] >= 0x7F800000u) return -2;  // (finite and > 0)
    }
    const uint64_t n_vals = row_off[num_rows];
    if ((n_vals && !row_vals) || n_vals > (uint64_t(1) << 31)) return -2;
    for (uint64_t k = 0; k < n_vals; ++k)
        if (row_vals[k] >= num_texts) return -2;
    try {
        std::vector<std::pair<uint32_t, uint32_t>> picked;
        vq::debug_text_rank(row_off, row_vals, row_score_bits, num_rows, num_texts, top_n, picked, out_touched);
        for (size_t k = 0; k < picked.size(); ++k) {
            out_texts[k] = picked[k].first;
            out_score_bits[k] = picked[k].second;
        }
        *out_n = uint32_t(picked.size());
    } catch (const std::exception&) {
        return -1;
    }
    return 0;
}
/* self-check (tests): the scans' column boost (apply_col_boost) alone on a caller's column, docs and scores; the boost is parsed as the compiler
   parses a request's (fill_boost_params).  0; -1 without a device; -2 for arguments the parse or the kernel does not take */
int vq_debug_col_boost(int fun, float param, const char* expression, const float* skip, uint32_t n_skip, const float* values, uint32_t num_keys,
                       const uint32_t* present_words, uint32_t key_base, const uint32_t* docs, const float* scores, uint32_t n, float* out_scores,
                       float* out_log10_factor) {
    if (fun < BF_NONE || fun > BF_REPLACE || (n_skip && !skip) || (num_keys && !values) || !docs || !scores || !out_scores || !out_log10_factor || n == 0 ||
        n > (uint32_t(1) << 24) || num_keys > (uint32_t(1) << 24) || uint64_t(key_base) + num_keys > 0xFFFFFFFFull)
        return -2;
    DColBoost cb{};
    try {
        vqreq::RequestBoostPart b;
        if (fun != BF_NONE) b.boost_fun = vqreq::BoostFunction(fun);  // enum order matches BoostFun
        b.param = param;
        if (n_skip) b.skip_when_score = std::vector<float>(skip, skip + n_skip);
        if (expression) b.expression = std::string(expression);
        fill_boost_params(cb, b);
    } catch (const std::exception& e) {
        g_err = e.what();  // (a bad expression, more than 4 skip values)
        return -2;
    }
    return vq::debug_col_boost(cb, values, num_keys, present_words, key_base, docs, scores, n, out_scores, out_log10_factor);
}
/* self-check (tests): the facet top-`top` kernels on a caller's histogram */
int vq_debug_facet_select(const uint32_t* hist, uint32_t num_values, uint32_t top, uint32_t misalign, uint32_t* out_values, uint32_t* out_counts) {
    if (!hist || !out_values || !out_counts) return -1;
    return vq::debug_facet_select(hist, num_values, top, misalign, out_values, out_counts);
}
/* self-checks (tests): k_merge_spans / k_finalize alone on crafted key tables, all jobs in one launch.  0; -1 on a device error; -2 for
   arguments outside the documented ranges, decided before the device is touched */
static bool debug_merge_jobs_ok(const uint32_t* top_k, const uint32_t* n_spans, uint32_t n_jobs, uint64_t tables, uint64_t* keys_out) {
    if (!top_k || !n_jobs || !tables) return false;
    uint64_t keys = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        if (top_k[j] == 0 || top_k[j] > uint32_t(vq::kMaxTopK) || (n_spans && n_spans[j] == 0)) return false;
        keys += uint64_t(n_spans ? n_spans[j] : 1) * top_k[j] * tables;
        if (keys > (uint64_t(1) << 24)) return false;
    }
    *keys_out = keys;
    return true;
}
int vq_debug_merge_spans(const uint64_t* span_keys, const uint32_t* n_spans, const uint32_t* top_k, uint32_t n_jobs, uint64_t* out_keys) {
    uint64_t keys = 0;
    if (!span_keys || !n_spans || !out_keys || !debug_merge_jobs_ok(top_k, n_spans, n_jobs, 1, &keys)) return -2;
    try {
        vq::debug_merge_spans(span_keys, n_spans, top_k, n_jobs, out_keys);
    } catch (const std::exception&) {
        return -1;
    }
    return 0;
}
int vq_debug_finalize(const uint64_t* shard_keys, const uint64_t* shard_hits, uint32_t num_shards, size_t stride_pad, const uint32_t* top_k, uint32_t n_jobs,
                      uint32_t* out_ids, uint32_t* out_score_bits, uint32_t* out_n, uint64_t* out_hits) {
    uint64_t keys = 0;
    if (!shard_keys || !shard_hits || !out_ids || !out_score_bits || !out_n || !out_hits || stride_pad % 8 != 0 || stride_pad > (size_t(1) << 20) ||
        !debug_merge_jobs_ok(top_k, nullptr, n_jobs, num_shards, &keys))
        return -2;
    try {
        vq::debug_finalize(shard_keys, shard_hits, num_shards, stride_pad, top_k, n_jobs, out_ids, out_score_bits, out_n, out_hits);
    } catch (const std::exception&) {
        return -1;
    }
    return 0;
}

/* self-checks (tests): the pre-pass drivers of prepass.cpp alone — the jobs described as the compiler describes them, run by run_*_jobs, every
   job's whole (doc, f32) list copied back with its 8 sentinel entries.  0; -1 without a device (or when the driver fails); -2 for arguments
   outside the documented ranges */

int vq_debug_union_lists(const vq_index* index, const char* const* store_paths, const uint64_t* job_off, const uint32_t* tokens, const uint32_t* term_score_bits,
                         uint32_t n_jobs, int route, uint64_t out_cap, uint32_t* out_len, uint32_t* out_max_bits, uint32_t* out_docs, uint32_t* out_val_bits) {
    if (!index || !n_jobs || !store_paths || !debug_csr_ok(job_off, tokens, n_jobs) || !term_score_bits || route < 0 || route > 2 || !out_len || !out_max_bits ||
        !out_docs || !out_val_bits)
        return -2;
    UnionTable table;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        auto it = store_paths[j] ? index->idx->postings.find(store_paths[j]) : index->idx->postings.end();
        if (it == index->idx->postings.end()) return -2;
        const uint64_t n = job_off[j + 1] - job_off[j];
        if (n == 0 || (route == 1 && n > 64 * 64)) return -2;  // (the compiler asks for no union without lists; two levels of k_union take 64 x 64)
        UnionJob job;
        job.key = debug_job_key(j);
        for (uint64_t k = job_off[j]; k < job_off[j + 1]; ++k) {
            if (tokens[k] >= it->second.num_tokens) return -2;
            UnionJob::Term t{&it->second, tokens[k], 0.0f};
            std::memcpy(&t.score, &term_score_bits[k], 4);
            job.terms.push_back(t);
        }
        table.emplace(job.key, std::move(job));
    }
    return debug_run(index, [&](Workspace& ws, hipStream_t st) {
        vq::run_union_jobs(*index->idx, ws, table, st, route == 0 ? -1 : route == 1 ? 64 * 64 : 0);
        std::vector<const UnionJob*> jobs;
        for (auto& kv : table) jobs.push_back(&kv.second);
        for (uint32_t j = 0; j < n_jobs; ++j) {
            out_len[j] = jobs[j]->len;
            std::memcpy(&out_max_bits[j], &jobs[j]->max_value, 4);
        }
        return debug_copy_lists(jobs, out_cap, out_docs, out_val_bits);
    });
}

int vq_debug_locality_lists(const vq_index* index, const char* const* t2t_paths, const char* const* t2a_paths, const uint64_t* job_off, const uint32_t* tokens,
                            uint32_t n_jobs, uint64_t out_cap, uint32_t* out_len, uint32_t* out_docs, uint32_t* out_val_bits) {
    if (!index || !n_jobs || !t2t_paths || !t2a_paths || !debug_csr_ok(job_off, tokens, n_jobs) || !out_len || !out_docs || !out_val_bits) return -2;
    LocalityTable table;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        auto t2t = t2t_paths[j] ? index->idx->kv.find(t2t_paths[j]) : index->idx->kv.end();
        auto t2a = t2a_paths[j] ? index->idx->kv.find(t2a_paths[j]) : index->idx->kv.end();
        // the images the driver reads: the token -> text table as a CSR, the text -> anchor rows with their row table
        if (t2t == index->idx->kv.end() || t2a == index->idx->kv.end() || !t2t->second.text_csr || !t2a->second.list_rows || !t2a->second.d_row_start.p) return -2;
        LocalityJob job;
        job.key = debug_job_key(j);
        job.t2t_path = t2t_paths[j];
        job.t2a_path = t2a_paths[j];
        job.tokens.assign(tokens + job_off[j], tokens + job_off[j + 1]);
        table.emplace(job.key, std::move(job));
    }
    return debug_run(index, [&](Workspace& ws, hipStream_t st) {
        vq::run_locality_jobs(*index->idx, ws, table, st);
        std::vector<const LocalityJob*> jobs;
        for (auto& kv : table) jobs.push_back(&kv.second);
        for (uint32_t j = 0; j < n_jobs; ++j) out_len[j] = jobs[j]->len;
        return debug_copy_lists(jobs, out_cap, out_docs, out_val_bits);
    });
}

int vq_debug_range_hits(const vq_index* index, const char* const* store_paths, const uint64_t* token_off, const uint32_t* tokens, const uint64_t* anchor_off,
                        const uint32_t* anchors, uint32_t n_jobs, uint64_t* out_counts) {
    if (!index || !n_jobs || !store_paths || !debug_csr_ok(token_off, tokens, n_jobs) || !debug_csr_ok(anchor_off, anchors, n_jobs) || !out_counts) return -2;
    if (index->idx->sharded() && !index->idx->allreduce_fn) return -2;  // (the driver sums the counts over the shards)
    RangeTable table;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        auto it = store_paths[j] ? index->idx->postings.find(store_paths[j]) : index->idx->postings.end();
        if (it == index->idx->postings.end()) return -2;
        RangeJob job;
        job.key = debug_job_key(j);
        job.store_path = store_paths[j];
        job.tokens.assign(tokens + token_off[j], tokens + token_off[j + 1]);
        for (uint32_t t : job.tokens)
            if (t >= it->second.num_tokens) return -2;
        auto an = std::make_shared<std::vector<uint32_t>>(anchors + anchor_off[j], anchors + anchor_off[j + 1]);
        for (size_t k = 0; k < an->size(); ++k)
            if ((*an)[k] == 0xFFFFFFFFu || (k && (*an)[k - 1] >= (*an)[k])) return -2;
        job.anchors = std::move(an);
        table.emplace(job.key, std::move(job));
    }
    return debug_run(index, [&](Workspace& ws, hipStream_t st) {
        vq::run_range_jobs(*index->idx, ws, table, UnionTable(), st);
        uint64_t at = 0;
        for (auto& kv : table) {
            std::copy(kv.second.counts.begin(), kv.second.counts.end(), out_counts + at);
            at += kv.second.counts.size();
        }
        return true;
    });
}

int vq_debug_boost1n_lists(const vq_index* index, const char* const* to_parent_paths, const char* const* to_anchor_paths, const char* const* boost_paths,
                           const uint64_t* job_off, const uint32_t* text_ids, uint32_t n_jobs, uint64_t out_cap, uint32_t* out_len, uint32_t* out_total,
                           uint32_t* out_flags, uint32_t* out_docs, uint32_t* out_val_bits) {
    if (!index || !n_jobs || !to_parent_paths || !to_anchor_paths || !boost_paths || !debug_csr_ok(job_off, text_ids, n_jobs) || !out_len || !out_total || !out_flags ||
        !out_docs || !out_val_bits)
        return -2;
    Boost1nTable table;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        auto tp = to_parent_paths[j] ? index->idx->kv.find(to_parent_paths[j]) : index->idx->kv.end();
        auto ta = to_anchor_paths[j] ? index->idx->kv.find(to_anchor_paths[j]) : index->idx->kv.end();
        auto bc = boost_paths[j] ? index->idx->boost.find(boost_paths[j]) : index->idx->boost.end();
        // the images the driver reads: both tables as whole CSRs in HBM
        if (tp == index->idx->kv.end() || ta == index->idx->kv.end() || bc == index->idx->boost.end() || !tp->second.value_csr || !ta->second.value_csr) return -2;
        Boost1nJob job;
        job.key = debug_job_key(j);
        job.to_parent_path = to_parent_paths[j];
        job.to_anchor_path = to_anchor_paths[j];
        job.boost_path = boost_paths[j];
        job.text_ids.assign(text_ids + job_off[j], text_ids + job_off[j + 1]);
        table.emplace(job.key, std::move(job));
    }
    return debug_run(index, [&](Workspace& ws, hipStream_t st) {
        vq::run_boost1n_jobs(*index->idx, ws, table, st);
        std::vector<const Boost1nJob*> jobs;
        for (auto& kv : table) jobs.push_back(&kv.second);
        for (uint32_t j = 0; j < n_jobs; ++j) {
            out_len[j] = jobs[j]->len;
            out_total[j] = jobs[j]->total;
            out_flags[j] = (jobs[j]->ascending ? 1u : 0u) | (jobs[j]->several ? 2u : 0u);
        }
        return debug_copy_lists(jobs, out_cap, out_docs, out_val_bits);
    });
}

}  // extern "C"
