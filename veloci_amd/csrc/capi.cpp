// extern "C" boundary (include/veloci_amd.h).  No torch types, no exceptions across the ABI.  The hooks that drive a kernel or a pre-pass alone:
// capi_debug.cpp; the communicator and the sharded step: shard_step.cpp; what the three share: capi_internal.hpp.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <functional>
#include <future>

#include "capi_internal.hpp"
#include "text.hpp"

using namespace vq;
using vqreq::Request;
using vqreq::VelociError;

thread_local std::string vq::g_err;

int vq::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

namespace {
void json_f32(std::string& out, float f) {
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.9g", double(f));
    out += buf;
    if (!std::strpbrk(buf, ".eEni")) out += ".0";
}
}  // namespace

static void explain_json(std::string& s, const Result& R) {
    s += '[';
    for (size_t i = 0; i < R.explain.size(); ++i) {
        if (i) s += ',';
        s += R.explain[i].first ? explain_records_json(R.explain[i].second) : std::string("null");
    }
    s += ']';
}
static void why_found_terms_json(std::string& s, const std::map<std::string, std::vector<std::string>>& m) {
    s += '{';
    bool first = true;
    for (auto& kv : m) {
        if (!first) s += ',';
        first = false;
        vqjson::escape_to(s, kv.first);
        s += ":[";
        for (size_t i = 0; i < kv.second.size(); ++i) {
            if (i) s += ',';
            vqjson::escape_to(s, kv.second[i]);
        }
        s += ']';
    }
    s += '}';
}

static void why_found_info_json(std::string& s, const Result& R) {  // {"<anchor id>": {"<field>": ["highlighted text", ...]}}
    s += '{';
    bool first = true;
    for (auto& [anchor, fields] : R.why_found_info) {
        if (!first) s += ',';
        first = false;
        s += '"' + std::to_string(anchor) + "\":";
        why_found_terms_json(s, fields);
    }
    s += '}';
}

// ---- canonical dump of a parsed request: every field of search::Request in declaration order, absent options as null, f32 values as their bit
// patterns — what the parser understood, for the golden request-parse fixtures (tests/golden/request_parse.json)
namespace {
void dump_f32(std::string& s, float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    s += std::to_string(b);
}
template <class T, class F>
void dump_opt(std::string& s, const std::optional<T>& v, F f) {
    if (v) f(s, *v);
    else s += "null";
}
void dump_usize(std::string& s, size_t v) { s += std::to_string(v); }
void dump_bool(std::string& s, bool v) { s += v ? "true" : "false"; }
void dump_str(std::string& s, const std::string& v) { vqjson::escape_to(s, v); }
void dump_boost_part(std::string& s, const vqreq::RequestBoostPart& b) {
    static const char* const names[] = {"Log2", "Log10", "Multiply", "Add", "Replace"};
    s += "{\"path\":";
    dump_str(s, b.path);
    s += ",\"boost_fun\":";
    if (b.boost_fun) s += std::string("\"") + names[int(*b.boost_fun)] + "\"";
    else s += "null";
    s += ",\"param\":";
    dump_opt(s, b.param, dump_f32);
    s += ",\"skip_when_score\":";
    if (b.skip_when_score) {
        s += '[';
        for (size_t i = 0; i < b.skip_when_score->size(); ++i) {
            if (i) s += ',';
            dump_f32(s, (*b.skip_when_score)[i]);
        }
        s += ']';
    } else s += "null";
    s += ",\"expression\":";
    dump_opt(s, b.expression, dump_str);
    s += '}';
}
void dump_boost_list(std::string& s, const std::optional<std::vector<vqreq::RequestBoostPart>>& v) {
    if (!v) {
        s += "null";
        return;
    }
    s += '[';
    for (size_t i = 0; i < v->size(); ++i) {
        if (i) s += ',';
        dump_boost_part(s, (*v)[i]);
    }
    s += ']';
}
void dump_options(std::string& s, const std::optional<vqreq::SearchRequestOptions>& o) {
    if (!o) {
        s += "null";
        return;
    }
    s += "{\"explain\":";
    dump_bool(s, o->explain);
    s += ",\"top\":";
    dump_opt(s, o->top, dump_usize);
    s += ",\"skip\":";
    dump_opt(s, o->skip, dump_usize);
    s += ",\"boost\":";
    dump_boost_list(s, o->boost);
    s += '}';
}
void dump_part(std::string& s, const vqreq::RequestSearchPart& p) {
    s += "{\"path\":";
    dump_str(s, p.path);
    s += ",\"terms\":[";
    for (size_t i = 0; i < p.terms.size(); ++i) {
        if (i) s += ',';
        dump_str(s, p.terms[i]);
    }
    s += "],\"levenshtein_distance\":";
    if (p.levenshtein_distance) s += std::to_string(*p.levenshtein_distance);
    else s += "null";
    s += ",\"starts_with\":";
    dump_bool(s, p.starts_with);
    s += ",\"is_regex\":";
    dump_bool(s, p.is_regex);
    s += ",\"token_value\":";
    if (p.token_value) dump_boost_part(s, *p.token_value);
    else s += "null";
    s += ",\"boost\":";
    dump_opt(s, p.boost, dump_f32);
    s += ",\"ignore_case\":";
    dump_opt(s, p.ignore_case, dump_bool);
    s += ",\"snippet\":";
    dump_opt(s, p.snippet, dump_bool);
    s += ",\"snippet_info\":";
    dump_bool(s, p.has_snippet_info);
    s += ",\"top\":";
    dump_opt(s, p.top, dump_usize);
    s += ",\"skip\":";
    dump_opt(s, p.skip, dump_usize);
    s += ",\"options\":";
    dump_options(s, p.options);
    s += '}';
}
void dump_search_request(std::string& s, const vqreq::SearchRequest& r) {
    if (r.kind == vqreq::SearchRequest::Search) {
        s += "{\"search\":";
        dump_part(s, r.part);
        s += '}';
        return;
    }
    s += r.kind == vqreq::SearchRequest::Or ? "{\"or\":{\"queries\":[" : "{\"and\":{\"queries\":[";
    for (size_t i = 0; i < r.tree.queries.size(); ++i) {
        if (i) s += ',';
        dump_search_request(s, r.tree.queries[i]);
    }
    s += "],\"options\":";
    dump_options(s, r.tree.options);
    s += "}}";
}
void dump_parts(std::string& s, const std::optional<std::vector<vqreq::RequestSearchPart>>& v) {
    if (!v) {
        s += "null";
        return;
    }
    s += '[';
    for (size_t i = 0; i < v->size(); ++i) {
        if (i) s += ',';
        dump_part(s, (*v)[i]);
    }
    s += ']';
}
}  // namespace

// ---- between a batch of request handles and the flat outputs (capi_internal.hpp)
// the requests behind the handles of a batch (a null handle stays null: that request alone fails)
std::vector<const Request*> vq::request_pointers(const vq_request* const* requests, size_t n) {
    std::vector<const Request*> reqs(n);
    for (size_t i = 0; i < n; ++i) reqs[i] = requests[i] ? requests[i]->req.get() : nullptr;
    return reqs;
}
void vq::keep_requests(PartialBatch& pb, const vq_request* const* requests, size_t n) {
    pb.owners.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (requests[i]) pb.owners[i] = requests[i]->req;
}
// Explain records and why_found_info (why_found with select) are produced by vq_search / vq_search_json / vq_search_batch: the flat outputs have no
// place for them, and on the sharded path a rank only holds the postings and the texts of its own docs.
void vq::decline_explain(std::vector<std::unique_ptr<Result>>& results, std::vector<int>& st, std::vector<std::string>& errs, const char* where) {
    for (size_t i = 0; i < results.size(); ++i)
        if (st[i] == 0 && results[i] && (results[i]->explain_plan || results[i]->why_found_plan)) {
            st[i] = VQ_ERR_UNSUPPORTED;
            errs[i] = std::string("unsupported on the MI355X query path: ") + (results[i]->explain_plan ? "explain on " : "why_found with select on ") + where;
            results[i].reset();
        }
}
// the flat merges rank top + skip <= kMaxTopK per request (vq_merge_partials hands page 0 back instead: vq_result_is_page / vq_request_page_after)
void vq::decline_deep(std::vector<std::unique_ptr<Result>>& results, std::vector<int>& st, std::vector<std::string>& errs) {
    for (size_t i = 0; i < results.size(); ++i)
        if (st[i] == 0 && results[i] && results[i]->deep) {
            st[i] = VQ_ERR_UNSUPPORTED;
            errs[i] = "unsupported on the MI355X query path: top + skip > " + std::to_string(vq::kMaxTopK) + " on the sharded partial / merge path";
            results[i].reset();
        }
}
void vq::copy_flat(const std::vector<std::unique_ptr<Result>>& results, const std::vector<int>& st, const std::vector<std::string>& errs, size_t base,
                   size_t stride, uint64_t* num_hits, uint32_t* counts, uint32_t* ids, float* scores, int* status) {
    for (size_t k = 0; k < results.size(); ++k) {
        const size_t i = base + k;
        if (status) status[i] = st[k];
        num_hits[i] = 0;
        counts[i] = 0;
        if (st[k] != 0) {
            if (g_err.empty()) g_err = errs[k];
            continue;
        }
        const Result& r = *results[k];
        if (r.ids.size() > stride) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "flat output: stride smaller than a request's top");
        num_hits[i] = r.num_hits;
        counts[i] = uint32_t(r.ids.size());
        if (r.ids.empty()) continue;  // (an empty vector's data() may be null: not an argument for memcpy)
        std::memcpy(ids + i * stride, r.ids.data(), r.ids.size() * 4);
        std::memcpy(scores + i * stride, r.scores.data(), r.scores.size() * 4);
    }
}

extern "C" {

const char* vq_last_error(void) { return g_err.c_str(); }
const char* vq_version(void) { return "veloci_amd 0.5 (gfx950)"; }
/* self-check (tests): inputs for which the kernels' fast a/100 differs from the correctly rounded division, over all f16 values */
uint32_t vq_debug_div100_mismatches(void) { return vq::debug_div100_mismatches(); }
/* tools/probe_occupancy.py (like the stamp readers below: exported, not part of the header): LDS bytes of a probe kernel's one-wave workgroup (shape: kProbe* of kernels.hpp; nd / na operands beside the cover / probed as arrays; arr_slot words per
   array operand) and how many of them the runtime keeps resident on a CU */
uint32_t vq_debug_probe_occupancy(uint32_t shape, uint32_t nd, uint32_t na, uint32_t arr_slot, uint32_t cand_cap, uint32_t* lds_bytes) {
    const size_t lds = vq::scan_probe_lds_bytes(cand_cap, nd, na, arr_slot);
    if (lds_bytes) *lds_bytes = uint32_t(lds);
    return vq::debug_probe_occupancy(shape, lds);
}
/* tests, tools: requests that ran a second time because a speculative route's result could not be confirmed (k_scan_probe_or) */
uint64_t vq_index_speculative_reruns(const vq_index* index) { return index ? index->idx->or_reruns.load() : 0; }
/* tests, tools: since the index was built, the probes of suggest batches that k_dict_topn answered and the match records those batches copied back
   (a top-n probe: min(its matches, top + skip + 200) entries) */
void vq_index_suggest_topn_probes(const vq_index* index, uint64_t* topn_probes, uint64_t* records_copied_back) {
    if (topn_probes) *topn_probes = index ? index->idx->suggest_topn_probes.load() : 0;
    if (records_copied_back) *records_copied_back = index ? index->idx->suggest_records_back.load() : 0;
}
/* tests, tools: since the index was built, the parts of highlight batches whose texts were ranked on the device and the snippets those batches built */
void vq_index_highlight_rank_counts(const vq_index* index, uint64_t* device_parts, uint64_t* snippets_built) {
    if (device_parts) *device_parts = index ? index->idx->highlight_device_parts.load() : 0;
    if (snippets_built) *snippets_built = index ? index->idx->highlight_snippets_built.load() : 0;
}

// ------------------------------------------------------------------ index
vq_index_builder* vq_index_builder_new(uint32_t num_anchors, uint32_t doc_lo, uint32_t doc_hi) {
    auto* b = new vq_index_builder();
    b->b.num_anchors = num_anchors;
    b->b.doc_lo = doc_lo;
    b->b.doc_hi = doc_hi;
    return b;
}
void vq_index_builder_free(vq_index_builder* b) { delete b; }

int vq_index_add_fst(vq_index_builder* b, const char* path, uint32_t num_terms, const uint8_t* term_bytes, const uint64_t* term_offsets) {
    return guard([&] {
        if (!b || !path || (num_terms && (!term_bytes || !term_offsets))) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_add_fst: null argument");
        HostFst f;
        f.terms.reserve(num_terms);
        for (uint32_t i = 0; i < num_terms; ++i) {
            f.terms.emplace_back(reinterpret_cast<const char*>(term_bytes) + term_offsets[i], size_t(term_offsets[i + 1] - term_offsets[i]));
            if (i && !(f.terms[i - 1] < f.terms[i])) throw VelociError(VQ_ERR_INVALID_ARGUMENT, std::string("terms must be bytewise sorted and unique: ") + path);
        }
        b->b.fst[path] = std::move(f);
    });
}

int vq_index_add_token_to_anchor_score(vq_index_builder* b, const char* path, uint32_t num_tokens, const uint64_t* offsets, const uint32_t* anchors,
                                       const uint32_t* scores, const uint64_t* global_lens) {
    return guard([&] {
        if (!b || !path || !offsets) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_add_token_to_anchor_score: null argument");
        HostPostings p;
        p.offsets.assign(offsets, offsets + num_tokens + 1);
        const uint64_t n = offsets[num_tokens];
        if (n && (!anchors || !scores)) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_add_token_to_anchor_score: null arrays");
        // copied and checked on host_threads() threads (billions of postings at the bench's scale)
        p.anchors.resize(n);
        p.scores.resize(n);
        const size_t piece = size_t(1) << 24;
        parallel_for((n + piece - 1) / piece, host_threads(), [&](size_t i) {
            const size_t off = i * piece, m = std::min<size_t>(piece, n - off);
            std::memcpy(p.anchors.data() + off, anchors + off, m * 4);
            std::memcpy(p.scores.data() + off, scores + off, m * 4);
        });
        parallel_for(num_tokens, host_threads(), [&](size_t t) {
            for (uint64_t i = offsets[t] + 1; i < offsets[t + 1]; ++i)
                if (!(anchors[i - 1] < anchors[i])) throw VelociError(VQ_ERR_INVALID_ARGUMENT, std::string("posting lists must be ascending and unique: ") + path);
        });
        if (global_lens) p.global_lens.assign(global_lens, global_lens + num_tokens);
        b->b.postings[path] = std::move(p);
    });
}

int vq_index_add_key_value_store(vq_index_builder* b, const char* path, uint32_t key_base, uint32_t num_keys, const uint64_t* offsets,
                                 const uint32_t* values) {
    return guard([&] {
        if (!b || !path || !offsets) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_add_key_value_store: null argument");
        HostKV k;
        k.key_base = key_base;
        k.offsets.assign(offsets, offsets + num_keys + 1);
        const uint64_t n = offsets[num_keys];
        if (n && !values) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_add_key_value_store: null values");
        k.values.assign(values, values + n);
        b->b.kv[path] = std::move(k);
    });
}

int vq_index_add_phrase_pair_to_anchor(vq_index_builder* b, const char* path, uint64_t num_pairs, const uint32_t* t1, const uint32_t* t2,
                                       const uint64_t* offsets, const uint32_t* anchors) {
    return guard([&] {
        if (!b || !path || !offsets) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_add_phrase_pair_to_anchor: null argument");
        HostPhrase p;
        p.t1.assign(t1, t1 + num_pairs);
        p.t2.assign(t2, t2 + num_pairs);
        p.offsets.assign(offsets, offsets + num_pairs + 1);
        p.anchors.assign(anchors, anchors + offsets[num_pairs]);
        b->b.phrase[path] = std::move(p);
    });
}

int vq_index_add_boost(vq_index_builder* b, const char* path, uint32_t key_base, uint32_t num_keys, const uint8_t* present, const uint32_t* value_bits) {
    return guard([&] {
        if (!b || !path || (num_keys && !value_bits)) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_add_boost: null argument");
        HostBoost h;
        h.key_base = key_base;
        if (present) h.present.assign(present, present + num_keys);
        h.bits.assign(value_bits, value_bits + num_keys);
        b->b.boost[path] = std::move(h);
    });
}

int vq_index_set_column_meta(vq_index_builder* b, const char* field, int is_anchor_identity_column, int tokenize) {
    return guard([&] {
        if (!b || !field) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_set_column_meta: null argument");
        ColumnMeta m;
        m.is_anchor_identity_column = is_anchor_identity_column != 0;
        m.tokenize = tokenize != 0;
        b->b.columns[field] = m;
    });
}

int vq_index_build(vq_index_builder* b, int device, vq_index** out) {
    return guard([&] {
        if (!b || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_build: null argument");
        *out = nullptr;
        auto idx = build_index(b->b, device);
        auto* h = new vq_index();
        h->idx = std::move(idx);
        *out = h;
    });
}
void vq_index_free(vq_index* i) { delete i; }

int vq_index_set_stream(vq_index* i, void* hip_stream) {
    return guard([&] {
        if (!i) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_set_stream: null index");
        std::vector<std::unique_lock<std::mutex>> quiet;  // no batch in flight
        for (auto& w : i->idx->ws) quiet.emplace_back(w.mu);
        i->idx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : i->idx->own_stream;
        i->idx->fin_stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : i->idx->own_fin_stream;
    });
}
int vq_index_set_streams(vq_index* i, void* scan_stream, void* finish_stream) {
    return guard([&] {
        if (!i) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_set_streams: null index");
        if (!scan_stream || !finish_stream) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_set_streams: null stream (vq_index_set_stream(index, NULL) restores the index's own)");
        std::vector<std::unique_lock<std::mutex>> quiet;  // no batch in flight
        for (auto& w : i->idx->ws) quiet.emplace_back(w.mu);
        i->idx->stream = static_cast<hipStream_t>(scan_stream);
        i->idx->fin_stream = static_cast<hipStream_t>(finish_stream);
    });
}
int vq_index_set_allreduce(vq_index* i, vq_allreduce_u64_fn fn, void* ctx) {
    return guard([&] {
        if (!i) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_index_set_allreduce: null index");
        std::vector<std::unique_lock<std::mutex>> quiet;  // no batch in flight
        for (auto& w : i->idx->ws) quiet.emplace_back(w.mu);
        i->idx->allreduce_fn = fn;
        i->idx->allreduce_ctx = ctx;
    });
}
uint64_t vq_index_device_bytes(const vq_index* i) { return i ? i->idx->device_bytes : 0; }

// ------------------------------------------------------------------ requests
int vq_request_parse(const char* json, size_t len, vq_request** out) {
    return guard([&] {
        if (!json || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_request_parse: null argument");
        *out = nullptr;
        auto r = std::make_unique<vq_request>();
        r->req = std::make_shared<Request>(vqreq::request_from_json_text(json, len));
        *out = r.release();
    });
}
int vq_request_has_facets(const vq_request* r) { return r && r->req->facets && !r->req->facets->empty() ? 1 : 0; }
const char* vq_request_to_json(const vq_request* r) {
    thread_local std::string s;
    s.clear();
    if (!r) return "null";
    const Request& q = *r->req;
    s += "{\"search_req\":";
    if (q.search_req) dump_search_request(s, *q.search_req);
    else s += "null";
    s += ",\"suggest\":";
    dump_parts(s, q.suggest);
    s += ",\"boost\":";
    dump_boost_list(s, q.boost);
    s += ",\"boost_term\":";
    dump_parts(s, q.boost_term);
    s += ",\"facets\":";
    if (q.facets) {
        s += '[';
        for (size_t i = 0; i < q.facets->size(); ++i) {
            if (i) s += ',';
            s += "{\"field\":";
            dump_str(s, (*q.facets)[i].field);
            s += ",\"top\":";
            dump_opt(s, (*q.facets)[i].top, dump_usize);
            s += '}';
        }
        s += ']';
    } else s += "null";
    s += ",\"phrase_boosts\":";
    if (q.phrase_boosts) {
        s += '[';
        for (size_t i = 0; i < q.phrase_boosts->size(); ++i) {
            if (i) s += ',';
            s += "{\"search1\":";
            dump_part(s, (*q.phrase_boosts)[i].search1);
            s += ",\"search2\":";
            dump_part(s, (*q.phrase_boosts)[i].search2);
            s += '}';
        }
        s += ']';
    } else s += "null";
    s += ",\"select\":";
    dump_bool(s, q.has_select);
    s += ",\"filter\":";
    if (q.filter) dump_search_request(s, *q.filter);
    else s += "null";
    s += ",\"top\":";
    dump_opt(s, q.top, dump_usize);
    s += ",\"skip\":";
    dump_opt(s, q.skip, dump_usize);
    s += ",\"why_found\":";
    dump_bool(s, q.why_found);
    s += ",\"text_locality\":";
    dump_bool(s, q.text_locality);
    s += ",\"explain\":";
    dump_bool(s, q.explain);
    s += '}';
    return s.c_str();
}
// Unicode lowercasing as the dictionary side applies it (str::to_lowercase, search_field.rs:284,312): for the code-point sweep against an
// independent implementation (tests/test_request_parse.py).  Returns the length, or (size_t)-1 when `cap` is too small.
size_t vq_debug_to_lowercase(const char* utf8, size_t len, char* out, size_t cap) {
    const std::string low = vqtext::to_lower_utf8(std::string(utf8 ? utf8 : "", utf8 ? len : 0));
    if (low.size() > cap) return size_t(-1);
    std::memcpy(out, low.data(), low.size());
    return low.size();
}
// util::normalize_text (src/util.rs:11-29) as vq_highlight_json applies it to the terms: checked against an independent regex engine by
// tests/test_request_parse.py.  Returns the length, or (size_t)-1 when `cap` is too small.
size_t vq_debug_normalize_text(const char* utf8, size_t len, char* out, size_t cap) {
    const std::string norm = vqtext::normalize_text(std::string(utf8 ? utf8 : "", utf8 ? len : 0));
    if (norm.size() > cap) return size_t(-1);
    std::memcpy(out, norm.data(), norm.size());
    return norm.size();
}
// The request compiler's id-list sort (ascending, duplicate-free, in place; returns the new length): a bitmap over dense id spans, radix passes over
// sparse ones, std::sort for short lists — swept against numpy by tests/test_request_parse.py.
size_t vq_debug_sort_unique_u32(uint32_t* ids, size_t n) { return ids || !n ? vq::debug_sort_unique(ids, n) : 0; }
// Compile `request` against `index` without launching anything: 0 when the query is ready to scan, negative when a pre-pass would run first
// (-1 union / locality jobs, -2 count pre-pass, -3 range jobs), or the error code the search would return (message in vq_last_error).  Host-only work —
// what the CPU sanitizer build exercises, and what tools/compile_bench.py times.
int vq_debug_compile(const vq_index* index, const vq_request* request) {
    int status = 0;
    const int rc = guard([&] {
        if (!index || !request) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_debug_compile: null argument");
        vq::CompiledQuery cq = vq::compile_query(*index->idx, *request->req);
        status = cq.status;
        if (cq.status != 0) g_err = cq.error;
    });
    return rc != 0 ? rc : status;
}
// The route a regex part (a RequestSearchPart as JSON, is_regex true) takes on `index`: 0 and the sizes of its DFA when k_dict_regex answers it,
// VQ_ERR_UNSUPPORTED with the reason in vq_last_error when it stays on the host route, or the error a search with the part would return.
int vq_debug_regex_compile(const vq_index* index, const char* part_json, size_t len, uint32_t* states, uint32_t* classes) {
    return guard([&] {
        if (!index || !part_json) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_debug_regex_compile: null argument");
        vqreq::RequestSearchPart part;
        try {
            part = vqreq::search_part_from_json(vqjson::parse(part_json, len));
        } catch (const vqjson::ParseError& e) {
            throw VelociError(VQ_ERR_JSON, std::string("JsonError: ") + e.what());
        }
        const vqregex::Compiled c = vq::regex_route(*index->idx, part);
        if (!c.device) throw VelociError(VQ_ERR_UNSUPPORTED, "regex leaf on the host route: " + c.reason);
        if (states) *states = c.dfa.n_states;
        if (classes) *classes = c.dfa.n_classes;
    });
}
void vq_request_free(vq_request* r) { delete r; }

// ------------------------------------------------------------------ doc sets
int vq_docset_create(const vq_index* index, const uint32_t* ids, uint64_t n, int ids_on_device, vq_docset** out) {
    return guard([&] {
        if (!index || !out || (n && !ids)) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_create: null argument");
        *out = nullptr;
        auto set = vq::make_docset(*index->idx, ids, n, ids_on_device != 0);
        auto* h = new vq_docset();
        h->set = std::move(set);
        *out = h;
    });
}
int vq_docset_from_filter(const vq_index* index, const char* filter_json, size_t len, const vq_docset* within, vq_docset** out) {
    return guard([&] {
        if (!index || !filter_json || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_from_filter: null argument");
        *out = nullptr;
        std::optional<vqreq::SearchRequest> filter;
        try {
            filter = vqreq::search_request_from_json(vqjson::parse(filter_json, len));
        } catch (const vqjson::ParseError& e) {
            throw VelociError(VQ_ERR_JSON, std::string("JsonError: ") + e.what());
        }
        auto set = vq::make_docset_from_filter(*index->idx, *filter, within ? within->set : nullptr);
        auto* h = new vq_docset();
        h->set = std::move(set);
        *out = h;
    });
}
int vq_docset_combine(const vq_index* index, int op, const vq_docset* const* sets, size_t n, vq_docset** out) {
    return guard([&] {
        if (!index || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_combine: null argument");
        *out = nullptr;
        if (!n || !sets) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_combine: no operands");
        std::vector<std::shared_ptr<const DocSet>> operands(n);  // held for the length of the call
        for (size_t i = 0; i < n; ++i) {
            if (!sets[i]) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_combine: operand " + std::to_string(i) + " is null");
            operands[i] = sets[i]->set;
        }
        auto set = vq::combine_docsets(*index->idx, op, operands);
        auto* h = new vq_docset();
        h->set = std::move(set);
        *out = h;
    });
}
int vq_docset_from_ranges(const vq_index* index, const char* ranges_json, size_t len, const vq_docset* within, vq_docset** out) {
    return guard([&] {
        if (!index || !ranges_json || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_from_ranges: null argument");
        *out = nullptr;
        std::vector<vq::RangeClause> clauses;
        try {
            clauses = vq::range_clauses_from_json(vqjson::parse(ranges_json, len));
        } catch (const vqjson::ParseError& e) {
            throw VelociError(VQ_ERR_JSON, std::string("JsonError: ") + e.what());
        }
        auto set = vq::make_docset_from_ranges(*index->idx, clauses, within ? within->set : nullptr);
        auto* h = new vq_docset();
        h->set = std::move(set);
        *out = h;
    });
}
int vq_debug_docset_range_route(const vq_docset* d) { return d ? d->set->range_route : -1; }
uint64_t vq_docset_ids(const vq_docset* d, uint32_t* out, uint64_t cap, int out_on_device) {
    if (!d) return 0;
    uint64_t n = 0;
    if (guard([&] { n = vq::copy_docset_ids(*d->set, out, cap, out_on_device != 0); }) != VQ_OK) return 0;  // (the reason is in vq_last_error)
    return n;
}
int vq_docset_facets(const vq_index* index, const vq_docset* d, const char* facets_json, size_t len, vq_result** out) {
    return guard([&] {
        if (!index || !d || !facets_json || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_facets: null argument");
        *out = nullptr;
        std::vector<vqreq::FacetRequest> facets;
        try {
            const vqjson::Value v = vqjson::parse(facets_json, len);
            if (!v.is_null()) facets = vqreq::facets_from_json(v);  // (Request::facets is an Option: null is no facet)
        } catch (const vqjson::ParseError& e) {
            throw VelociError(VQ_ERR_JSON, std::string("JsonError: ") + e.what());
        }
        const std::shared_ptr<const DocSet> set = d->set;  // held for the length of the call
        auto res = vq::docset_facets(*index->idx, *set, facets);
        auto* h = new vq_result();
        h->r = std::move(*res);
        *out = h;
    });
}
float vq_debug_docset_facets_count_ms(void) { return vq::docset_facets_last_count_ms(); }
int vq_docset_aggregate(const vq_index* index, const vq_docset* d, const char* aggs_json, size_t len, vq_docset_aggs** out) {
    return guard([&] {
        if (!index || !d || !aggs_json || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_aggregate: null argument");
        *out = nullptr;
        std::vector<vq::AggSpec> specs;
        try {
            specs = vq::agg_specs_from_json(vqjson::parse(aggs_json, len));
        } catch (const vqjson::ParseError& e) {
            throw VelociError(VQ_ERR_JSON, std::string("JsonError: ") + e.what());
        }
        const std::shared_ptr<const DocSet> set = d->set;  // held for the length of the call
        auto h = std::make_unique<vq_docset_aggs>();
        h->r = vq::docset_aggregate(*index->idx, *set, specs);
        for (const vq::AggResult& a : h->r)
            h->c.push_back(vq_docset_agg{a.docs, a.count, a.missing, a.nan, a.sum, a.min, a.max, uint64_t(a.buckets.size()), a.buckets.empty() ? nullptr : a.buckets.data()});
        *out = h.release();
    });
}
size_t vq_docset_aggs_len(const vq_docset_aggs* a) { return a ? a->c.size() : 0; }
const vq_docset_agg* vq_docset_aggs_get(const vq_docset_aggs* a, size_t i) { return a && i < a->c.size() ? &a->c[i] : nullptr; }
void vq_docset_aggs_free(vq_docset_aggs* a) { delete a; }
float vq_debug_docset_aggregate_ms(void) { return vq::docset_aggregate_last_ms(); }
int vq_docset_top_by(const vq_index* index, const vq_docset* d, const char* spec_json, size_t len, vq_docset_top** out) {
    return guard([&] {
        if (!index || !d || !spec_json || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_top_by: null argument");
        *out = nullptr;
        vq::TopSpec spec;
        try {
            spec = vq::top_spec_from_json(vqjson::parse(spec_json, len));
        } catch (const vqjson::ParseError& e) {
            throw VelociError(VQ_ERR_JSON, std::string("JsonError: ") + e.what());
        }
        const std::shared_ptr<const DocSet> set = d->set;  // held for the length of the call
        auto h = std::make_unique<vq_docset_top>();
        h->r = vq::docset_top(*index->idx, *set, spec);
        *out = h.release();
    });
}
size_t vq_docset_top_len(const vq_docset_top* t) { return t ? t->r.docs.size() : 0; }
const uint32_t* vq_docset_top_docs(const vq_docset_top* t) { return t ? t->r.docs.data() : nullptr; }
const float* vq_docset_top_values(const vq_docset_top* t) { return t ? t->r.values.data() : nullptr; }
const uint8_t* vq_docset_top_kinds(const vq_docset_top* t) { return t ? t->r.kinds.data() : nullptr; }
void vq_docset_top_counters(const vq_docset_top* t, uint64_t* out4) {
    if (!out4) return;
    out4[0] = t ? t->r.n_docs : 0;
    out4[1] = t ? t->r.count : 0;
    out4[2] = t ? t->r.nan : 0;
    out4[3] = t ? t->r.missing : 0;
}
int vq_docset_top_is_partial(const vq_docset_top* t) { return t && t->r.partial ? 1 : 0; }
int vq_docset_top_merge(const vq_docset_top* const* parts, size_t n, vq_docset_top** out) {
    return guard([&] {
        if (!out || (n && !parts)) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_top_merge: null argument");
        *out = nullptr;
        std::vector<const vq::TopResult*> p(n);
        for (size_t i = 0; i < n; ++i) p[i] = parts[i] ? &parts[i]->r : nullptr;
        auto h = std::make_unique<vq_docset_top>();
        h->r = vq::docset_top_merge(p);
        *out = h.release();
    });
}
size_t vq_docset_top_pack(const vq_docset_top* t, uint8_t* out, size_t cap) {
    if (!t) return 0;
    size_t need = 0;
    if (guard([&] {
            const std::vector<uint8_t> image = vq::docset_top_pack(t->r);
            need = image.size();
            if (out && cap >= need) std::memcpy(out, image.data(), need);
        }) != VQ_OK)
        return 0;  // (the reason is in vq_last_error)
    return need;
}
int vq_docset_top_unpack(const uint8_t* bytes, size_t len, vq_docset_top** out) {
    return guard([&] {
        if (!bytes || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_docset_top_unpack: null argument");
        *out = nullptr;
        auto h = std::make_unique<vq_docset_top>();
        h->r = vq::docset_top_unpack(bytes, len);
        *out = h.release();
    });
}
void vq_docset_top_free(vq_docset_top* t) { delete t; }
float vq_debug_docset_top_ms(void) { return vq::docset_top_last_ms(); }
int vq_debug_docset_route(const vq_docset* d) { return d ? d->set->route : -1; }
uint64_t vq_docset_len(const vq_docset* d) { return d ? d->set->len : 0; }
uint64_t vq_docset_local_len(const vq_docset* d) { return d ? d->set->local_len : 0; }
uint64_t vq_docset_device_bytes(const vq_docset* d) { return d ? d->set->device_bytes : 0; }
uint64_t vq_debug_docset_part(const vq_docset* d, int part, uint32_t* out, uint64_t cap) {
    if (!d) return 0;
    const DocSet& s = *d->set;
    const DevBuf* src = nullptr;
    uint64_t count = 0;
    switch (part) {
        case 0: src = &s.docs; count = s.local_len; break;
        case 1: src = &s.bitmap; count = s.bitmap_words; break;
        case 2: src = &s.rank_dir; count = s.rank_entries; break;
        case 3: src = &s.tile_dir; count = s.tile_entries; break;
        case 4: src = &s.docs; count = (uint64_t(s.local_len) + 3u) & ~uint64_t(3); break;
        default: return 0;
    }
    const uint64_t take = std::min(count, cap);
    if (take && out && src->p && hipMemcpy(out, src->p, take * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return count;
}
int vq_debug_docset_timings(const vq_docset* d, float* ms_mark, float* ms_count_scan, float* ms_expand) {
    if (!d || d->set->ms_mark < 0.0f) return -1;
    if (ms_mark) *ms_mark = d->set->ms_mark;
    if (ms_count_scan) *ms_count_scan = d->set->ms_count_scan;
    if (ms_expand) *ms_expand = d->set->ms_expand;
    return 0;
}
void vq_docset_free(vq_docset* d) { delete d; }
int vq_request_set_docset(vq_request* r, const vq_docset* d) {
    return guard([&] {
        if (!r) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_request_set_docset: null request");
        // a batch or step in flight shares the request: it keeps the request, and the set, it was begun with — the handle goes on with a copy
        if (r->req.use_count() > 1) r->req = std::make_shared<Request>(*r->req);
        r->req->docset = d ? d->set : nullptr;  // (a copy of the shared_ptr: the request keeps the set alive)
    });
}
// The continuation of `request` behind the ranked hit (score, id): what a caller of the sharded partial / merge path sends for the next page of a
// request whose top + skip reaches beyond one scan's ranking (vq_result_is_page).
int vq_request_page_after(const vq_request* request, float score, uint32_t id, vq_request** out) {
    return guard([&] {
        if (!request || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_request_page_after: null argument");
        auto r = std::make_unique<vq_request>();
        r->req = std::make_shared<Request>(vq::page_request_after(*request->req, score, id));
        *out = r.release();
    });
}

// ------------------------------------------------------------------ results
uint64_t vq_result_num_hits(const vq_result* r) { return r->r.num_hits; }
int vq_result_is_page(const vq_result* r) { return r->r.deep ? 1 : 0; }
uint64_t vq_result_execution_time_ns(const vq_result* r) { return r->r.execution_time_ns; }
size_t vq_result_len(const vq_result* r) { return r->r.ids.size(); }
const uint32_t* vq_result_ids(const vq_result* r) { return r->r.ids.data(); }
const float* vq_result_scores(const vq_result* r) { return r->r.scores.data(); }
size_t vq_result_num_facets(const vq_result* r) { return r->r.facets.size(); }
const char* vq_result_facet_field(const vq_result* r, size_t f) { return r->r.facets[f].field.c_str(); }
size_t vq_result_facet_len(const vq_result* r, size_t f) { return r->r.facets[f].entries.size(); }
const char* vq_result_facet_value(const vq_result* r, size_t f, size_t i) { return r->r.facets[f].entries[i].first.c_str(); }
uint64_t vq_result_facet_count(const vq_result* r, size_t f, size_t i) { return r->r.facets[f].entries[i].second; }
const char* vq_result_to_json(const vq_result* r) {
    std::string& s = r->r.json;
    s.clear();
    s += "{\"execution_time_ns\":" + std::to_string(r->r.execution_time_ns) + ",\"num_hits\":" + std::to_string(r->r.num_hits) + ",\"data\":[";
    for (size_t i = 0; i < r->r.ids.size(); ++i) {
        if (i) s += ',';
        s += "{\"id\":" + std::to_string(r->r.ids[i]) + ",\"score\":";
        json_f32(s, r->r.scores[i]);
        s += '}';
    }
    s += "],\"ids\":[]";
    if (r->r.has_facets) {
        s += ",\"facets\":{";
        for (size_t f = 0; f < r->r.facets.size(); ++f) {
            if (f) s += ',';
            vqjson::escape_to(s, r->r.facets[f].field);
            s += ":[";
            for (size_t i = 0; i < r->r.facets[f].entries.size(); ++i) {
                if (i) s += ',';
                s += '[';
                vqjson::escape_to(s, r->r.facets[f].entries[i].first);
                s += ',' + std::to_string(r->r.facets[f].entries[i].second) + ']';
            }
            s += ']';
        }
        s += '}';
    }
    if (r->r.has_explain) {
        s += ",\"explain\":";
        explain_json(s, r->r);
    }
    if (!r->r.why_found_terms.empty()) {
        s += ",\"why_found_terms\":";
        why_found_terms_json(s, r->r.why_found_terms);
    }
    if (r->r.why_found_plan) {
        s += ",\"why_found_info\":";
        why_found_info_json(s, r->r);
    }
    s += '}';
    return s.c_str();
}
const char* vq_result_explain_json(const vq_result* r) {
    thread_local std::string s;
    s.clear();
    if (!r->r.has_explain) return "null";
    explain_json(s, r->r);
    return s.c_str();
}
const char* vq_result_why_found_terms_json(const vq_result* r) {
    thread_local std::string s;
    s.clear();
    why_found_terms_json(s, r->r.why_found_terms);
    return s.c_str();
}
const char* vq_result_why_found_info_json(const vq_result* r) {
    thread_local std::string s;
    s.clear();
    if (!r->r.why_found_plan) return "null";
    why_found_info_json(s, r->r);
    return s.c_str();
}
void vq_result_free(vq_result* r) { delete r; }

// ------------------------------------------------------------------ suggest
// the text of a suggest request: a Request with "suggest" parts, or a bare RequestSearchPart
static Request suggest_request_from_text(const char* json, size_t len) {
    Request req;
    try {
        vqjson::Value v = vqjson::parse(json, len);
        if (v.is_object() && v.get("suggest")) req = vqreq::request_from_json(v);
        else {  // a bare RequestSearchPart: search_field::suggest (:221-231), top / skip are the part's
            vqreq::RequestSearchPart part = vqreq::search_part_from_json(v);
            req.suggest = std::vector<vqreq::RequestSearchPart>{part};
            req.top = part.top;
            req.skip = part.skip;
        }
    } catch (const vqjson::ParseError& e) {
        throw VelociError(VQ_ERR_JSON, std::string("JsonError: ") + e.what());
    }
    return req;
}
int vq_suggest_json(const vq_index* index, const char* json, size_t len, vq_suggest_result** out) {
    return guard([&] {
        if (!index || !json || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_suggest_json: null argument");
        *out = nullptr;
        const Request req = suggest_request_from_text(json, len);
        auto* r = new vq_suggest_result();
        try {
            r->e = run_suggest(*index->idx, req);
        } catch (...) {
            delete r;
            throw;
        }
        *out = r;
    });
}
int vq_suggest_batch(const vq_index* index, const char* const* json, const size_t* len, size_t n, vq_suggest_result** out, int* status) {
    std::string first_error;
    const int rc = guard([&] {
        if (!index || (n && (!json || !len || !out))) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_suggest_batch: null argument");
        for (size_t i = 0; i < n; ++i) out[i] = nullptr;
        std::vector<Request> parsed(n);
        std::vector<const Request*> reqs(n, nullptr);
        std::vector<int> parse_status(n, 0);
        std::vector<std::string> parse_error(n);
        for (size_t i = 0; i < n; ++i) {
            try {
                if (!json[i]) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_suggest_batch: null request text");
                parsed[i] = suggest_request_from_text(json[i], len[i]);
                reqs[i] = &parsed[i];
            } catch (const VelociError& e) {
                parse_status[i] = e.code;
                parse_error[i] = e.what();
            }
        }
        std::vector<std::vector<SuggestEntry>> results;
        std::vector<int> st;
        std::vector<std::string> errs;
        run_suggest_batch(*index->idx, reqs.data(), n, results, st, errs);
        for (size_t i = 0; i < n; ++i) {
            const int code = parse_status[i] ? parse_status[i] : st[i];
            if (status) status[i] = code;
            if (code == 0) {
                auto* r = new vq_suggest_result();
                r->e = std::move(results[i]);
                out[i] = r;
            } else if (first_error.empty()) first_error = parse_status[i] ? parse_error[i] : errs[i];
        }
    });
    if (rc == VQ_OK && !first_error.empty()) g_err = first_error;  // (the batch ran: the first failing request's text)
    return rc;
}
int vq_highlight_json(const vq_index* index, const char* json, size_t len, vq_suggest_result** out) {
    return guard([&]() {
        if (!index || !json || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_highlight_json: null argument");
        *out = nullptr;
        vqreq::RequestSearchPart part;
        try {
            part = vqreq::search_part_from_json(vqjson::parse(json, len));
        } catch (const vqjson::ParseError& e) {
            throw VelociError(VQ_ERR_JSON, std::string("JsonError: ") + e.what());
        }
        auto* r = new vq_suggest_result();
        try {
            r->e = run_highlight(*index->idx, std::move(part));
        } catch (...) {
            delete r;
            throw;
        }
        *out = r;
    });
}
int vq_highlight_batch(const vq_index* index, const char* const* json, const size_t* len, size_t n, vq_suggest_result** out, int* status) {
    std::string first_error;
    const int rc = guard([&] {
        if (!index || (n && (!json || !len || !out))) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_highlight_batch: null argument");
        for (size_t i = 0; i < n; ++i) out[i] = nullptr;
        std::vector<vqreq::RequestSearchPart> parsed(n);
        std::vector<const vqreq::RequestSearchPart*> parts(n, nullptr);
        std::vector<int> parse_status(n, 0);
        std::vector<std::string> parse_error(n);
        for (size_t i = 0; i < n; ++i) {
            try {
                if (!json[i]) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_highlight_batch: null request text");
                try {
                    parsed[i] = vqreq::search_part_from_json(vqjson::parse(json[i], len[i]));
                } catch (const vqjson::ParseError& e) {
                    throw VelociError(VQ_ERR_JSON, std::string("JsonError: ") + e.what());
                }
                parts[i] = &parsed[i];
            } catch (const VelociError& e) {
                parse_status[i] = e.code;
                parse_error[i] = e.what();
            }
        }
        std::vector<std::vector<SuggestEntry>> results;
        std::vector<int> st;
        std::vector<std::string> errs;
        run_highlight_batch(*index->idx, parts.data(), n, results, st, errs);
        for (size_t i = 0; i < n; ++i) {
            const int code = parse_status[i] ? parse_status[i] : st[i];
            if (status) status[i] = code;
            if (code == 0) {
                auto* r = new vq_suggest_result();
                r->e = std::move(results[i]);
                out[i] = r;
            } else if (first_error.empty()) first_error = parse_status[i] ? parse_error[i] : errs[i];
        }
    });
    if (rc == VQ_OK && !first_error.empty()) g_err = first_error;  // (the batch ran: the first failing part's text)
    return rc;
}
// highlight_text (highlight_field.rs:92-146).  Returns the snippet's byte length (written to `out` when it fits `cap`), VQ_HIGHLIGHT_NONE when there is
// nothing to highlight, VQ_HIGHLIGHT_ERROR on an error (vq_last_error); a length above `cap` means: call again with a larger buffer.
size_t vq_highlight_text(const char* text, size_t len, const char* const* terms, const size_t* term_lens, size_t n_terms, const char* snippet_info_json, size_t json_len,
                         int tokenized, char* out, size_t cap) {
    size_t result = size_t(-2);
    guard([&] {
        if ((!text && len) || (!terms && n_terms) || (!out && cap)) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_highlight_text: null argument");
        vqreq::SnippetInfo opt;
        if (snippet_info_json && json_len) {
            try {
                opt = vqreq::snippet_info_from_json(vqjson::parse(snippet_info_json, json_len));
            } catch (const vqjson::ParseError& e) {
                throw VelociError(VQ_ERR_JSON, std::string("JsonError: ") + e.what());
            }
        }
        std::vector<std::string> set;
        for (size_t i = 0; i < n_terms; ++i) set.emplace_back(terms[i] ? terms[i] : "", terms[i] ? (term_lens ? term_lens[i] : std::strlen(terms[i])) : 0);
        const std::optional<std::string> sn = vq::highlight_text(std::string(text ? text : "", len), set, opt, tokenized != 0);
        if (!sn) {
            result = size_t(-1);
            return;
        }
        if (sn->size() <= cap) std::memcpy(out, sn->data(), sn->size());
        result = sn->size();
    });
    return result;
}
size_t vq_suggest_len(const vq_suggest_result* r) { return r->e.size(); }
const char* vq_suggest_text(const vq_suggest_result* r, size_t i) { return r->e[i].text.c_str(); }
float vq_suggest_score(const vq_suggest_result* r, size_t i) { return r->e[i].score; }
uint32_t vq_suggest_term_id(const vq_suggest_result* r, size_t i) { return r->e[i].term_id; }
void vq_suggest_free(vq_suggest_result* r) { delete r; }

// ------------------------------------------------------------------ search
// does the batch have pre-passes (dictionary scans of fuzzy / prefix leaves, then unions, range jobs ...)?  Their syncs make the host side of a
// batch long; such batches are cut in two and run on two host threads (a sample decides: it is about the batch's character)
static bool batch_has_prepasses(const std::vector<const Request*>& reqs) {
    std::function<bool(const vqreq::SearchRequest&)> scans = [&](const vqreq::SearchRequest& r) {
        if (r.kind == vqreq::SearchRequest::Search) return vq::needs_dictionary_scan(r.part);
        for (auto& q : r.tree.queries)
            if (scans(q)) return true;
        return false;
    };
    for (size_t i = 0; i < reqs.size(); i += 16)
        if (reqs[i] && reqs[i]->search_req && scans(*reqs[i]->search_req)) return true;
    return false;
}
static int run_batch(const vq_index* index, const vq_request* const* requests, size_t n, vq_result** out, int* status, std::string* first_error) {
    const std::vector<const Request*> reqs = request_pointers(requests, n);
    std::vector<std::unique_ptr<Result>> results(n);
    std::vector<int> st(n, 0);
    std::vector<std::string> errs(n);
    auto run_range = [&](size_t b, size_t e) {
        std::vector<std::unique_ptr<Result>> r;
        std::vector<int> s2;
        std::vector<std::string> e2;
        {
            auto pb = run_partial(*index->idx, reqs.data() + b, e - b);
            finish_batch(*index->idx, *pb, nullptr, 1, r, s2, e2);
        }  // (the batch's workspace is free again: deep requests scan on)
        complete_deep_requests(*index->idx, reqs.data() + b, e - b, r, s2, e2);
        complete_explain_requests(*index->idx, r, s2, e2);
        complete_why_found_requests(*index->idx, r, s2, e2);
        for (size_t i = b; i < e; ++i) {
            results[i] = std::move(r[i - b]);
            st[i] = s2[i - b];
            errs[i] = std::move(e2[i - b]);
        }
    };
    // A batch with pre-passes waits for the device several times before its scan starts (dictionary scans, unions, range counts): cut in
    // two and run on two host threads, one half computes while the other waits (VQ_BATCH_HALVES=0: one piece)
    static const bool halves = !(std::getenv("VQ_BATCH_HALVES") && std::atoi(std::getenv("VQ_BATCH_HALVES")) == 0);
    if (halves && n >= 128 && kWorkspaces >= 2 && batch_has_prepasses(reqs)) {
        auto other = std::async(std::launch::async, run_range, n / 2, n);
        try {
            run_range(0, n / 2);
        } catch (...) {
            other.wait();
            throw;
        }
        other.get();
    } else run_range(0, n);
    for (size_t i = 0; i < n; ++i) {
        out[i] = nullptr;
        if (status) status[i] = st[i];
        if (st[i] == 0) {
            auto* r = new vq_result();
            r->r = std::move(*results[i]);
            out[i] = r;
        } else if (first_error && first_error->empty()) *first_error = errs[i];
    }
    return 0;
}

int vq_search(const vq_index* index, const vq_request* request, vq_result** out) {
    int st = 0;
    std::string err;
    int rc = guard([&] {
        if (!index || !request || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_search: null argument");
        *out = nullptr;
        const vq_request* arr[1] = {request};
        run_batch(index, arr, 1, out, &st, &err);
    });
    if (rc != VQ_OK) return rc;
    if (st != 0) return fail(st, err);
    return VQ_OK;
}

int vq_search_json(const vq_index* index, const char* json, size_t len, vq_result** out) {
    vq_request* req = nullptr;
    int rc = vq_request_parse(json, len, &req);
    if (rc != VQ_OK) return rc;
    rc = vq_search(index, req, out);
    vq_request_free(req);
    return rc;
}

int vq_search_batch(const vq_index* index, const vq_request* const* requests, size_t n, vq_result** out, int* status) {
    return guard([&] {
        if (!index || (n && (!requests || !out))) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_search_batch: null argument");
        std::string err;
        run_batch(index, requests, n, out, status, &err);
        if (!err.empty()) g_err = err;
    });
}

/* self-check (tests): what the count pre-pass measures for the requests of one batch — the batch's own compilation up to and including
   run_count_queries (exec.cpp debug_node_counts), no result scan.  Request i's measured nodes are entries node_off[i] .. node_off[i + 1] of
   node_ids / hits / hits_in_filter, in counter order.  0; -1 without a device (or when a pre-pass fails); -2 for arguments outside the documented
   ranges (a null pointer, n == 0, `out_cap` too small for the nodes) */
int vq_debug_node_counts(const vq_index* index, const vq_request* const* requests, size_t n, int summed, uint64_t out_cap, int* status, uint32_t* has_filter,
                         uint64_t* filter_count, uint32_t* n_spans, uint32_t* tile_words, uint64_t* node_off, uint32_t* node_ids, uint64_t* hits,
                         uint64_t* hits_in_filter) {
    if (!index || !n || !requests || summed < 0 || summed > 1 || !status || !has_filter || !filter_count || !n_spans || !tile_words || !node_off ||
        (out_cap && (!node_ids || !hits || !hits_in_filter)))
        return -2;
    try {
        const std::vector<const Request*> reqs = request_pointers(requests, n);
        const std::vector<vq::NodeCounts> counts = vq::debug_node_counts(*index->idx, reqs.data(), n, summed != 0);
        g_err.clear();
        uint64_t need = 0;
        for (const vq::NodeCounts& c : counts) need += c.nodes.size();
        if (need > out_cap) return -2;
        node_off[0] = 0;
        for (size_t i = 0; i < n; ++i) {
            const vq::NodeCounts& c = counts[i];
            status[i] = c.status;
            if (c.status > 0 && g_err.empty()) g_err = c.error;  // (the first failing request's text)
            has_filter[i] = c.has_filter ? 1u : 0u;
            filter_count[i] = c.filter_count;
            n_spans[i] = c.n_spans;
            tile_words[i] = c.tile_words;
            uint64_t at = node_off[i];
            for (const vq::NodeCounts::Node& nd : c.nodes) {
                node_ids[at] = nd.id;
                hits[at] = nd.hits;
                hits_in_filter[at] = nd.hits_in_filter;
                ++at;
            }
            node_off[i + 1] = at;
        }
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

int vq_search_batch_flat(const vq_index* index, const vq_request* const* requests, size_t n, size_t stride, uint64_t* num_hits, uint32_t* counts,
                         uint32_t* ids, float* scores, int* status) {
    return guard([&] {
        if (!index || (n && (!requests || !num_hits || !counts || !ids || !scores))) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_search_batch_flat: null argument");
        const std::vector<const Request*> reqs = request_pointers(requests, n);
        // Large batches run as a software pipeline of chunks over the index's two workspaces: while the GPU scans chunk c
        // the host compiles chunk c+1, and chunk c-1's merge + download run on the finish stream.
        bool any_deep = false;  // top + skip beyond one scan's ranking: such requests page on after their batch (not pipelined)
        for (size_t i = 0; i < n; ++i)
            if (reqs[i]) any_deep = any_deep || uint64_t(reqs[i]->top.value_or(10)) + uint64_t(reqs[i]->skip.value_or(0)) > uint64_t(vq::kMaxTopK);
        if (any_deep) {
            std::vector<std::unique_ptr<Result>> results;
            std::vector<int> st;
            std::vector<std::string> errs;
            {
                auto pb = run_partial(*index->idx, reqs.data(), n);
                finish_batch(*index->idx, *pb, nullptr, 1, results, st, errs);
            }
            complete_deep_requests(*index->idx, reqs.data(), n, results, st, errs);
            decline_explain(results, st, errs, "the flat batch path");
            copy_flat(results, st, errs, 0, stride, num_hits, counts, ids, scores, status);
            return;
        }
        static const size_t chunks_env = [] {
            const char* e = std::getenv("VQ_FLAT_CHUNKS");
            return size_t(e ? std::max(1, std::atoi(e)) : 0);
        }();
        // Requests with pre-passes (dictionary scans of fuzzy / prefix leaves, then unions) make the HOST side of a chunk long: it waits for
        // each pre-pass.  Two host threads, two chunks each, keep the GPU fed (config #4: 4.3 ms of kernels per chunk against 5 ms of
        // host-visible time; one thread: 50 k requests/s).  Plain batches stay on the calling thread: their host side is short.
        static const bool one_thread = std::getenv("VQ_FLAT_ONE_THREAD") != nullptr;
        static const size_t small_chunks = [] {  // a batch of 128 .. 511 requests with pre-passes: chunks of the two-thread pipeline (1: one piece)
            const char* e = std::getenv("VQ_FLAT_SMALL_CHUNKS");
            const int v = e ? std::atoi(e) : 2;
            return size_t(v == 4 ? 4 : v == 2 ? 2 : 1);
        }();
        const bool with_prepasses = kWorkspaces >= 4 && !one_thread && n >= 128 && batch_has_prepasses(reqs);
        // Plain batches on a large index: two chunks — the second is compiled while the first scans; launches of 256 requests fill the chip less
        // evenly than launches of 512 (100 M docs: 3-term AND 110.6 k requests/s with 2 chunks, 109.4 k with 1, 107.9 k with 4, 103.7 k with 8; the
        // request mix of config #5 68.5 k against 58.5 k).  On a small index the scan of a chunk is short next to its compilation and four chunks
        // hide more of the host side (10 M docs, AND + phrases + locality: 402 k with 4, 386 k with 2).
        const uint64_t shard_docs = uint64_t(index->idx->doc_hi) - index->idx->doc_lo;
        const size_t plain_chunks = shard_docs >= 32'000'000ull ? 2 : 4;
        const size_t nchunks = n >= 512 ? (chunks_env ? chunks_env : with_prepasses ? 4 : plain_chunks) : with_prepasses ? small_chunks : 1;
        std::vector<std::unique_ptr<PartialBatch>> inflight(nchunks);
        auto bounds = [&](size_t c) { return std::make_pair(n * c / nchunks, n * (c + 1) / nchunks); };
        auto finish = [&](size_t c) {
            std::vector<std::unique_ptr<Result>> results;
            std::vector<int> st;
            std::vector<std::string> errs;
            finish_batch(*index->idx, *inflight[c], nullptr, 1, results, st, errs);
            decline_explain(results, st, errs, "the flat batch path");
            copy_flat(results, st, errs, bounds(c).first, stride, num_hits, counts, ids, scores, status);
            inflight[c].reset();
        };
        const bool prepasses = with_prepasses && (nchunks == 4 || nchunks == 2);
        if (prepasses) {
            auto half = [&](size_t t) {
                for (size_t c = t; c < nchunks; c += 2) {
                    auto [b, e] = bounds(c);
                    inflight[c] = run_partial(*index->idx, reqs.data() + b, e - b, int(c));
                }
                for (size_t c = t; c < nchunks; c += 2) finish(c);
            };
            auto other = std::async(std::launch::async, half, size_t(1));
            try {
                half(0);
            } catch (...) {
                other.wait();
                throw;
            }
            other.get();
            return;
        }
        for (size_t c = 0; c < nchunks; ++c) {
            if (c >= size_t(kWorkspaces)) finish(c - kWorkspaces);
            auto [b, e] = bounds(c);
            inflight[c] = run_partial(*index->idx, reqs.data() + b, e - b, int(c % kWorkspaces));
        }
        for (size_t c = nchunks >= size_t(kWorkspaces) ? nchunks - kWorkspaces : 0; c < nchunks; ++c) finish(c);
    });
}

// ------------------------------------------------------------------ shard partials
int vq_search_batch_partial(const vq_index* index, const vq_request* const* requests, size_t n, vq_partial_batch** out) {
    return guard([&] {
        if (!index || !out || (n && !requests)) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_search_batch_partial: null argument");
        *out = nullptr;
        const std::vector<const Request*> reqs = request_pointers(requests, n);
        auto pb = run_partial(*index->idx, reqs.data(), n);
        keep_requests(*pb, requests, n);
        // on the index's own stream the packed buffer must be complete before another library (RCCL) reads it; on a
        // caller-provided stream the caller's collective is ordered behind the scan by the stream itself
        if (index->idx->stream == index->idx->own_stream) VQ_HIP(hipStreamSynchronize(index->idx->stream));
        auto* h = new vq_partial_batch();
        h->pb = std::move(pb);
        *out = h;
    });
}
// A chunk of a sharded step whose chunks share ONE collective: workspace `slot` (0 .. VQ_PARTIAL_SLOTS-1, one per chunk in flight), partial placed at
// `arena_offset` (a multiple of 256) of the index's partial arena.
int vq_search_batch_partial_at(const vq_index* index, const vq_request* const* requests, size_t n, int slot, size_t arena_offset, vq_partial_batch** out) {
    return guard([&] {
        if (!index || !out || (n && !requests)) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_search_batch_partial_at: null argument");
        if (slot < 0 || slot >= vq::kWorkspaces) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_search_batch_partial_at: slot out of range");
        *out = nullptr;
        const std::vector<const Request*> reqs = request_pointers(requests, n);
        auto pb = run_partial(*index->idx, reqs.data(), n, slot, int64_t(arena_offset));
        keep_requests(*pb, requests, n);
        if (index->idx->stream == index->idx->own_stream) VQ_HIP(hipStreamSynchronize(index->idx->stream));
        auto* h = new vq_partial_batch();
        h->pb = std::move(pb);
        *out = h;
    });
}
int vq_partial_slots(void) { return vq::kWorkspaces; }
void* vq_index_partial_arena_ptr(const vq_index* i) {
    if (!i) return nullptr;
    if (guard([&] {
            VQ_HIP(hipSetDevice(i->idx->device));
            i->idx->arena.ensure(vq::Index::kArenaBytes);
        }) != 0)
        return nullptr;
    return i->idx->arena.p;
}
size_t vq_partial_total_bytes(const vq_partial_batch* p) { return p ? size_t(p->pb->layout.bytes) : 0; }
size_t vq_partial_bytes(const vq_partial_batch* p) { return p ? size_t(p->pb->layout.off_hist) : 0; }
void* vq_partial_device_ptr(vq_partial_batch* p) { return p ? p->pb->d_partial : nullptr; }
size_t vq_partial_hist_bytes(const vq_partial_batch* p) { return p ? size_t(p->pb->layout.total_hist) * 4 : 0; }
void* vq_partial_hist_device_ptr(vq_partial_batch* p) { return p && p->pb->d_partial ? p->pb->d_partial + p->pb->layout.off_hist : nullptr; }

int vq_merge_partials(const vq_index* index, vq_partial_batch* local, const void* gathered_device, uint32_t num_shards, vq_result** out, int* status) {
    return guard([&] {
        if (!index || !local || !out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_merge_partials: null argument");
        std::vector<std::unique_ptr<Result>> results;
        std::vector<int> st;
        std::vector<std::string> errs;
        finish_batch(*index->idx, *local->pb, gathered_device, num_shards, results, st, errs);
        // (a request that reaches beyond one scan's ranking comes back as its page 0, vq_result_is_page: the caller pages on, on all shards)
        decline_explain(results, st, errs, "the sharded partial / merge path");
        for (size_t i = 0; i < results.size(); ++i) {
            out[i] = nullptr;
            if (status) status[i] = st[i];
            if (st[i] == 0) {
                auto* r = new vq_result();
                r->r = std::move(*results[i]);
                out[i] = r;
            } else if (g_err.empty()) g_err = errs[i];
        }
    });
}
int vq_merge_partials_flat(const vq_index* index, vq_partial_batch* local, const void* gathered_device, uint32_t num_shards, size_t stride,
                           uint64_t* num_hits, uint32_t* counts, uint32_t* ids, float* scores, int* status) {
    return guard([&] {
        if (!index || !local || !num_hits || !counts || !ids || !scores) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_merge_partials_flat: null argument");
        std::vector<std::unique_ptr<Result>> results;
        std::vector<int> st;
        std::vector<std::string> errs;
        finish_batch(*index->idx, *local->pb, gathered_device, num_shards, results, st, errs);
        decline_deep(results, st, errs);
        decline_explain(results, st, errs, "the sharded partial / merge path");
        copy_flat(results, st, errs, 0, stride, num_hits, counts, ids, scores, status);
    });
}
int vq_merge_partials_flat_strided(const vq_index* index, vq_partial_batch* local, const void* gathered_device, uint32_t num_shards, size_t shard_stride,
                                   size_t stride, uint64_t* num_hits, uint32_t* counts, uint32_t* ids, float* scores, int* status) {
    return guard([&] {
        if (!index || !local || !num_hits || !counts || !ids || !scores) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_merge_partials_flat_strided: null argument");
        std::vector<std::unique_ptr<Result>> results;
        std::vector<int> st;
        std::vector<std::string> errs;
        finish_batch(*index->idx, *local->pb, gathered_device, num_shards, results, st, errs, shard_stride);
        decline_deep(results, st, errs);
        decline_explain(results, st, errs, "the sharded partial / merge path");
        copy_flat(results, st, errs, 0, stride, num_hits, counts, ids, scores, status);
    });
}
void vq_partial_free(vq_partial_batch* p) { delete p; }


// ------------------------------------------------------------------ measurement
int vq_profile_enable(vq_index* i, int on) {
    return guard([&] {
        if (!i) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_profile_enable: null index");
        std::lock_guard<std::mutex> g(i->idx->profile_mutex);
        i->idx->profile.enabled = on != 0;
    });
}
static bool is_scan_kernel(int k) { return k >= K_SCAN_LEAF_F32 && k <= K_TILE_SCAN; }
int vq_profile_read(const vq_index* i, int reset, double* scan_kernel_ms, uint64_t* scan_launches, uint64_t* algorithmic_bytes) {
    return guard([&] {
        if (!i) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_profile_read: null index");
        std::lock_guard<std::mutex> g(i->idx->profile_mutex);
        Profile& p = i->idx->profile;
        double ms = 0;
        uint64_t algo = 0;
        for (int k = 0; k < K_COUNT_; ++k)
            if (is_scan_kernel(k)) {
                ms += p.k[k].ms;
                algo += p.k[k].algorithmic_bytes;
            }
        if (scan_kernel_ms) *scan_kernel_ms = ms;
        if (scan_launches) *scan_launches = p.batches;
        if (algorithmic_bytes) *algorithmic_bytes = algo;
        if (reset) p = Profile{p.enabled};
    });
}
const char* vq_profile_json(const vq_index* i, int reset) {
    thread_local std::string out;
    out = "{}";
    if (!i) return out.c_str();
    std::lock_guard<std::mutex> g(i->idx->profile_mutex);
    Profile& p = i->idx->profile;
    out = "{\"batches\":" + std::to_string(p.batches) + ",\"kernels\":{";
    bool first = true;
    for (int k = 0; k < K_COUNT_; ++k) {
        const KernelProfile& kp = p.k[k];
        if (!kp.launches) continue;
        char buf[512];
        std::snprintf(buf, sizeof buf, "%s\"%s\":{\"ms\":%.6f,\"launches\":%llu,\"layout_bytes\":%llu,\"algorithmic_bytes\":%llu,\"gathered_bytes\":%llu,\"queries\":%llu,\"scan\":%s}",
                      first ? "" : ",", kKernelNames[k], kp.ms, (unsigned long long)kp.launches, (unsigned long long)kp.layout_bytes,
                      (unsigned long long)kp.algorithmic_bytes, (unsigned long long)kp.gathered_bytes, (unsigned long long)kp.queries, is_scan_kernel(k) ? "true" : "false");
        out += buf;
        first = false;
    }
    out += "}}";
    if (reset) p = Profile{p.enabled};
    return out.c_str();
}

#ifdef VQ_STAMP
void vq_debug_stamps(unsigned long long* out, int reset) { vq::debug_read_stamps(out, reset); }
void vq_debug_probe_stamps(unsigned long long* out, int reset) { vq::debug_read_probe_stamps(out, reset); }
#endif

}  // extern "C"
