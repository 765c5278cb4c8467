// Dictionary side of a search part: the matched terms of a leaf and their scores (get_term_ids_in_field, search_field.rs:277-398), and the
// dictionary probes a batch collects before that can run — fuzzy, prefix and regex parts, answered by k_dict_scan / k_dict_regex / k_dict_topn
// under the keys that lookup_terms looks them up by.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <regex>

#include "compile_internal.hpp"
#include "term_lookup.hpp"
#include "text.hpp"

namespace vq {

using namespace vqreq;

namespace {

// search_field.rs:27-33
float default_score_for_distance(uint8_t distance, bool prefix_matches) {
    if (prefix_matches) return 2.0f / (std::log2(float(distance) + 1.0f) + 0.2f);
    return 2.0f / (float(distance) + 0.2f);
}

bool cp_eq(uint32_t a, uint32_t b, bool ci) { return a == b || (ci && vqtext::lower_cp(a) == vqtext::lower_cp(b)); }

// Distance the reference scores a dictionary hit with (search_field.rs:691-732): the scoring automaton is built
// over the lower-cased term with transpositions at cost one; beyond its maximum it falls back to the plain
// character Levenshtein distance in u8 (255 for strings of 255 bytes or more).
uint8_t scoring_distance(const std::string& lower_hit, const std::string& lower_term, uint32_t dfa_max) {
    if (lower_hit == lower_term) return 0;  // (both distances of equal strings: the exact-match leaf, the common case)
    const auto h = vqtext::decode_utf8(lower_hit), t = vqtext::decode_utf8(lower_term);
    const size_t n = h.size(), m = t.size(), w = m + 1;
    std::vector<uint32_t> osa((n + 1) * w), lev((n + 1) * w);
    for (size_t j = 0; j <= m; ++j) osa[j] = lev[j] = uint32_t(j);
    for (size_t i = 1; i <= n; ++i) {
        osa[i * w] = lev[i * w] = uint32_t(i);
        for (size_t j = 1; j <= m; ++j) {
            const uint32_t sub = h[i - 1] == t[j - 1] ? 0u : 1u;
            lev[i * w + j] = std::min({lev[(i - 1) * w + j] + 1, lev[i * w + j - 1] + 1, lev[(i - 1) * w + j - 1] + sub});
            uint32_t v = std::min({osa[(i - 1) * w + j] + 1, osa[i * w + j - 1] + 1, osa[(i - 1) * w + j - 1] + sub});
            if (i > 1 && j > 1 && h[i - 1] == t[j - 2] && h[i - 2] == t[j - 1]) v = std::min(v, osa[(i - 2) * w + j - 2] + 1);
            osa[i * w + j] = v;
        }
    }
    if (osa[n * w + m] <= dfa_max) return uint8_t(osa[n * w + m]);
    if (lower_hit.size() >= 255 || lower_term.size() >= 255) return 255;
    return uint8_t(lev[n * w + m]);
}

// levenshtein_distance after the clamp of search_field.rs:285-287 (0 when absent; the empty-term error is raised by the compiler)
uint32_t clamped_lev(const RequestSearchPart& p) {
    if (!p.levenshtein_distance) return 0;
    const size_t chars = vqtext::decode_utf8(vqtext::to_lower_utf8(p.terms.empty() ? std::string() : p.terms[0])).size();
    if (chars == 0) return 0;
    return std::min<uint32_t>(*p.levenshtein_distance, uint32_t(chars) - 1);
}

// expression.rs:48-95 — "x op y", x/y = $SCORE or a float
void parse_expression(const std::string& expression, DColBoost& cb) {
    struct Tok {
        int kind;  // 0 score, 1 float, 2.. operators (2 div, 3 mul, 4 add, 5 sub)
        float val;
    };
    std::vector<Tok> ops;
    std::string current;
    auto try_float = [](const std::string& s, float& out) {
        if (s.empty()) return false;
        char* end = nullptr;
        out = std::strtof(s.c_str(), &end);
        return end && *end == 0 && end != s.c_str();
    };
    for (char ch : expression) {
        if (ch == ' ') {
            float v;
            if (try_float(current, v)) ops.push_back({1, v});
            current.clear();
        } else current.push_back(ch);
        if (current == "+") ops.push_back({4, 0}), current.clear();
        else if (current == "-") ops.push_back({5, 0}), current.clear();
        else if (current == "/") ops.push_back({2, 0}), current.clear();
        else if (current == "*") ops.push_back({3, 0}), current.clear();
        else if (current == "$SCORE") ops.push_back({0, 0}), current.clear();
    }
    float v;
    if (try_float(current, v)) ops.push_back({1, v});
    if (ops.size() < 3 || ops[0].kind > 1 || ops[2].kind > 1 || ops[1].kind < 2)
        throw VelociError(ERR_INVALID_REQUEST, "InvalidRequest: \"bad score expression " + expression + "\" ");
    cb.expr_lkind = ops[0].kind;
    cb.expr_lval = ops[0].val;
    cb.expr_rkind = ops[2].kind;
    cb.expr_rval = ops[2].val;
    cb.expr_op = ops[1].kind == 2 ? EX_DIV : ops[1].kind == 3 ? EX_MUL : ops[1].kind == 4 ? EX_ADD : EX_SUB;
}

// The two std::wregex objects of a regex leaf (the yardstick of both routes: their flags, the wrapper, their errors)
std::wstring regex_widen(const std::string& u8) {
    std::wstring w;
    for (uint32_t cp : vqtext::decode_utf8(u8)) w.push_back(wchar_t(cp));
    return w;
}
void regex_objects(const RequestSearchPart& p, std::wregex& whole, std::wregex& anywhere) {
    try {
        const auto flags = std::regex::ECMAScript | (p.ignore_case.value_or(true) ? std::regex::icase : std::regex::ECMAScript);
        const std::wstring pat = regex_widen(p.terms[0]);
        whole = std::wregex(L"[\\s\\S]*?(?:" + pat + L")", flags);
        anywhere = std::wregex(pat, flags);
    } catch (const std::regex_error& e) {
        throw VelociError(ERR_INVALID_REQUEST, std::string("InvalidRequest: \"regex ") + e.what() + "\" ");
    }
}

// Regex leaf (search_field.rs:72-83), a HOST fallback for the dictionary side only (the postings of the matched terms stay on the device):
// regex-automata 0.1.9's dense DFA walks the term's bytes, unanchored at the start (its builder acts as if the pattern began with
// `(?s:.)*?`), and the term is accepted when the walk ENDS in a match state; `starts_with` accepts once any prefix did.  Restated over code
// points with std::wregex (ECMAScript grammar: the common subset of the two syntaxes; case-insensitivity beyond ASCII follows the C locale).
std::vector<uint32_t> regex_candidates(const Dictionary& dict, const RequestSearchPart& p) {
    std::wregex whole, anywhere;
    regex_objects(p, whole, anywhere);
    std::vector<uint32_t> out;
    for (uint32_t id = 0; id < dict.terms.size(); ++id) {
        const std::wstring w = regex_widen(dict.terms[id]);
        if (p.starts_with ? std::regex_search(w, anywhere) : std::regex_match(w, whole)) out.push_back(id);
    }
    return out;
}

}  // namespace

// get_term_ids_in_field (search_field.rs:277-398) — dictionary side only
void lookup_terms(const Index& idx, const FuzzyTable* fuzzy, bool topn_probes, Leaf& l, bool get_scores, bool get_ids) {
    PhaseTimer pt(0);
    const RequestSearchPart& p = *l.part;
    // (`snippet` / `snippet_info` are not looked at here: a search resolves token hits with resolve_token_hits_to_text_id_ids_only, plan_steps.rs:184 —
    //  snippets are made by search_field::highlight alone, search_field.rs:243 = vq_highlight_json)
    if (p.terms.empty()) throw VelociError(ERR_INVALID_REQUEST, "InvalidRequest: \"terms is empty\" ");
    l.path = p.path;
    if (!ends_with(l.path, TEXTINDEX)) l.path += TEXTINDEX;
    const std::string lower_term = vqtext::to_lower_utf8(p.terms[0]);
    uint32_t lev = 0;
    if (p.levenshtein_distance) {  // :285-287
        const auto lower_cps = vqtext::decode_utf8(lower_term);
        if (lower_cps.empty()) throw VelociError(ERR_INVALID_REQUEST, "InvalidRequest: \"empty term with levenshtein_distance\" ");
        lev = std::min<uint32_t>(*p.levenshtein_distance, uint32_t(lower_cps.size()) - 1);
    }
    auto dit = idx.dict.find(l.path);
    if (dit == idx.dict.end()) throw VelociError(ERR_FST_NOT_FOUND, "field does not exist " + l.path + " (fst not found)");
    const Dictionary& dict = dit->second;
    const bool ci = p.ignore_case.value_or(true);  // search_field.rs:88
    const bool query_ascii = vqtext::is_ascii(p.terms[0].data(), p.terms[0].size());
    std::vector<uint32_t> query_cps;  // decoded when a comparison needs code points
    std::vector<uint32_t> cand;
    const FuzzyProbe* probe = nullptr;
    const bool regex = p.is_regex;
    const bool scan = !regex && (lev != 0 || p.starts_with);
    if (regex) {  // match set from k_dict_regex when the batch's probes hold the leaf, else the host walk; scored on the host either way
        const FuzzyProbe* fp = nullptr;
        if (fuzzy) {
            auto it = fuzzy->find(fuzzy_key(p));
            if (it != fuzzy->end() && it->second.regex && it->second.answered && it->second.status == 0) fp = &it->second;
        }
        if (fp) cand = fp->matches;
        else cand = regex_candidates(dict, p);
    } else if (scan) {  // match set computed on the device before compilation (k_dict_scan), ascending == FST stream order
        const FuzzyProbe* fp = nullptr;
        if (fuzzy && topn_probes && p.top) {
            // A top-n probe of a suggest batch: `matches` / `scores` are the FINAL buffer of the loop below, made by k_dict_topn over the
            // same matches in the same order, and they pass through that loop unchanged.  The loop's cut needs size == top_n + 200 BEFORE a
            // push, which at most top_n + 200 entries in all never reach; so worst_score never rises, nothing is skipped, and the stable
            // sort behind the loop sees the very vector the full route would have built.
            auto it = fuzzy->find(topn_key(p));
            if (it != fuzzy->end() && it->second.top_n != 0) fp = &it->second;
        }
        if (fuzzy && !fp) {
            auto it = fuzzy->find(fuzzy_key(p));
            if (it != fuzzy->end()) fp = &it->second;
        }
        if (!fp) unsupported("levenshtein_distance > 0 / starts_with without a dictionary scan (internal)");
        if (fp->status != 0) throw VelociError(fp->status, fp->error);
        cand = fp->matches;
        probe = fp;
    } else if (ci) {
        auto it = dict.lower_map.find(lower_term);
        if (it != dict.lower_map.end()) cand = it->second;
    } else {
        auto it = std::lower_bound(dict.terms.begin(), dict.terms.end(), p.terms[0]);
        if (it != dict.terms.end() && *it == p.terms[0]) cand.push_back(uint32_t(it - dict.terms.begin()));
    }
    const bool limit_result = p.top.has_value();  // :292
    const size_t top_n_search = p.top.value_or(10) + p.skip.value_or(0);
    float worst_score = -std::numeric_limits<float>::max();
    const bool check_prefix = p.starts_with || lev != 0;  // :302
    for (size_t ci_ = 0; ci_ < cand.size(); ++ci_) {  // ascending ids == FST stream order
        const uint32_t id = cand[ci_];
        if (!scan && !regex) {
            const std::string& cand_term = dict.terms[id];
            bool eq = true;
            if (query_ascii && vqtext::is_ascii(cand_term.data(), cand_term.size())) {  // bytes are code points
                eq = cand_term.size() == p.terms[0].size();
                for (size_t i = 0; i < cand_term.size() && eq; ++i) eq = cp_eq(uint8_t(cand_term[i]), uint8_t(p.terms[0][i]), ci);
            } else {
                const auto cps = vqtext::decode_utf8(cand_term);
                if (query_cps.empty() && !p.terms[0].empty()) query_cps = vqtext::decode_utf8(p.terms[0]);
                eq = cps.size() == query_cps.size();
                for (size_t i = 0; i < cps.size() && eq; ++i) eq = cp_eq(cps[i], query_cps[i], ci);
            }
            if (!eq) continue;
        }
        if (get_ids) l.hits_ids.push_back(id);
        if (get_scores) {  // :304-354
            float score;
            if (probe) score = probe->scores[ci_];
            else {
                const std::string lower_hit = vqtext::to_lower_utf8(dict.terms[id]);
                const bool prefix_matches = check_prefix && lower_hit.compare(0, lower_term.size(), lower_term) == 0 && lower_hit.size() >= lower_term.size();
                score = default_score_for_distance(scoring_distance(lower_hit, lower_term, lev), prefix_matches);
            }
            if (limit_result) {
                if (score < worst_score) continue;  // (:324-327 returns before the term text is recorded)
                if (!l.hits_scores.empty() && l.hits_scores.size() == top_n_search + 200) {  // sort.rs:24-34
                    std::sort(l.hits_scores.begin(), l.hits_scores.end(), [](auto& a, auto& b) { return a.second == b.second ? a.first > b.first : a.second > b.second; });
                    l.hits_scores.resize(top_n_search);
                    // (top + skip == 0 keeps nothing: the reference panics on its empty vector; here the bound stays where it was and the
                    // truncation behind the loop leaves no hit)
                    if (!l.hits_scores.empty()) worst_score = l.hits_scores.back().second;
                }
            }
            l.hits_scores.push_back({id, score});
            if (part_explains(p)) {  // :334-343 (kept for hits a later top-n cut drops again, as in the reference)
                ExplainRec e;
                e.kind = ExplainRec::LevenshteinScore;
                e.a = score;
                e.term_id = id;
                e.text = dict.terms[id];
                l.explain[id] = ExplainRecs{e};
            }
        }
        if (l.return_term || l.store_term_texts)  // :347-353
            l.terms.push_back({id, l.return_term_lowercase ? vqtext::to_lower_utf8(dict.terms[id]) : dict.terms[id]});
    }
    if (p.boost)  // :359-364
        for (auto& h : l.hits_scores) h.second *= *p.boost;
    if (limit_result) {  // :373-376 (the reference's sort is unstable: tie order is unspecified there)
        std::stable_sort(l.hits_scores.begin(), l.hits_scores.end(), [](auto& a, auto& b) { return a.second > b.second; });
        if (l.hits_scores.size() > top_n_search) l.hits_scores.resize(top_n_search);
    }
}

// token_value (search_field.rs:391-395): add_boost (boost.rs:470-504) over the matched TERMS — the boost column is keyed by term id
// ("<path>.textindex.token_values.boost_valid_to_value", create/token_values_to_tokens.rs) and shapes the term scores before any
// posting is read.  Host arithmetic (glibc log10f / log2f, as the reference links them).
void apply_token_value(const Index& idx, const RequestBoostPart& tv, Leaf& l) {
    const std::string path = tv.path + TEXTINDEX + TOKEN_VALUES + BOOST_VALID_TO_VALUE;
    auto bit = idx.boost.find(path);
    if (bit == idx.boost.end()) throw VelociError(ERR_INDEX_NOT_FOUND, "Did not found path in indices " + path);
    DColBoost cb{};
    fill_boost_params(cb, tv);
    for (auto& h : l.hits_scores) {
        bool skip = false;
        for (uint32_t s = 0; s < cb.nskip; ++s) skip = skip || std::fabs(cb.skip[s] - h.second) < 0.00001f;
        float v;
        if (skip || !bit->second.host_value(h.first, &v)) continue;
        const float vp = v + cb.param;
        float score = h.second;
        switch (cb.fun) {  // apply_boost, boost.rs:283-377
            case BF_LOG10: score *= std::log10(vp); break;
            case BF_LOG2: score *= std::log2(vp); break;
            case BF_MULTIPLY: score *= vp; break;
            case BF_ADD: score += vp; break;
            case BF_REPLACE: score = vp; break;
            default: break;
        }
        if (cb.expr_op != EX_NONE) {
            const float a = cb.expr_lkind == 0 ? v : cb.expr_lval, b = cb.expr_rkind == 0 ? v : cb.expr_rval;
            score += cb.expr_op == EX_DIV ? a / b : cb.expr_op == EX_MUL ? a * b : cb.expr_op == EX_ADD ? a + b : a - b;
        }
        if (part_explains(*l.part)) {  // boost.rs:297-300, 371-374
            ExplainRec e;
            e.kind = ExplainRec::Boost;
            if (cb.fun == BF_LOG10) {
                e.a = std::log10(vp);
                l.explain[h.first].push_back(e);
            }
            e.a = score;
            l.explain[h.first].push_back(e);
        }
        h.second = score;
    }
}

void fill_boost_params(DColBoost& cb, const RequestBoostPart& b) {
    cb.fun = b.boost_fun ? int32_t(*b.boost_fun) : BF_NONE;  // enum order matches BoostFun
    cb.param = b.param.value_or(0.0f);
    if (b.skip_when_score) {
        if (b.skip_when_score->size() > size_t(kMaxSkipWhen)) unsupported("more than 4 skip_when_score values");
        cb.nskip = uint32_t(b.skip_when_score->size());
        for (size_t i = 0; i < b.skip_when_score->size(); ++i) cb.skip[i] = (*b.skip_when_score)[i];
    }
    cb.expr_op = EX_NONE;
    if (b.expression) parse_expression(*b.expression, cb);
}

float default_score_for_distance_host(uint8_t distance, bool prefix_matches) { return default_score_for_distance(distance, prefix_matches); }

// ---- dictionary scans requested by a batch (collected before compilation, answered by k_dict_scan)
std::string fuzzy_key(const RequestSearchPart& p) {
    std::string path = p.path;
    if (!ends_with(path, TEXTINDEX)) path += TEXTINDEX;
    std::string k;
    key_s(k, path);
    key_s(k, p.terms.empty() ? std::string() : p.terms[0]);
    k += std::to_string(clamped_lev(p)) + (p.starts_with ? "p" : "-") + (p.ignore_case ? (*p.ignore_case ? "T" : "F") : "N");
    if (p.is_regex) k += 'R';
    return k;
}
bool needs_dictionary_scan(const RequestSearchPart& p) { return !p.terms.empty() && !p.is_regex && (clamped_lev(p) != 0 || p.starts_with); }
std::string topn_key(const RequestSearchPart& p) { return fuzzy_key(p) + "#" + std::to_string(p.top.value_or(10)) + "+" + std::to_string(p.skip.value_or(0)); }

// VQ_NO_SUGGEST_TOPN=1: every part of a suggest batch keeps the full route (all matches back, the top-n loop on the host)
static bool suggest_topn_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("VQ_NO_SUGGEST_TOPN");
        return !(e && *e && std::string(e) != "0");
    }();
    return on;
}
// what run_fuzzy_probes decides per probe: k_dict_scan takes a 16-bit image and a query of <= 64 code points below U+10000, every other probe
// goes to k_dict_scan_wide; either scores a hit itself when the lower-cased term has at most 64 code points (k_dict_scan: all below U+10000)
// and the lower-cased image is exact
bool probe_scored_on_device(const Index& idx, const FuzzyProbe& fp) {
    const Dictionary& d = idx.dict.at(fp.path);
    bool wide = d.char_bytes != 2 || fp.query.size() > 64;
    for (uint32_t cp : fp.query) wide = wide || cp > 0xFFFFu;
    const auto lcps = vqtext::decode_utf8(fp.lower_term);
    bool ok = lcps.size() <= 64 && d.low_exact;
    if (!wide)
        for (uint32_t cp : lcps) ok = ok && cp <= 0xFFFFu;
    return ok;
}

// VQ_NO_REGEX_DEVICE=1: every regex leaf stays on the host route
static bool regex_device_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("VQ_NO_REGEX_DEVICE");
        return !(e && *e && std::string(e) != "0");
    }();
    return on;
}
vqregex::Compiled regex_route(const Index& idx, const RequestSearchPart& p) {
    if (!p.is_regex) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "not a regex part (is_regex is false)");
    if (p.terms.empty()) throw VelociError(ERR_INVALID_REQUEST, "InvalidRequest: \"terms is empty\" ");
    std::string path = p.path;
    if (!ends_with(path, TEXTINDEX)) path += TEXTINDEX;
    auto dit = idx.dict.find(path);
    if (dit == idx.dict.end()) throw VelociError(ERR_FST_NOT_FOUND, "field does not exist " + path + " (fst not found)");
    {  // first, always: an invalid pattern is the host route's error, word for word
        std::wregex whole, anywhere;
        regex_objects(p, whole, anywhere);
    }
    if (!regex_device_enabled()) {
        vqregex::Compiled c;
        c.reason = "VQ_NO_REGEX_DEVICE is set";
        return c;
    }
    const Dictionary& d = dit->second;
    return vqregex::compile(vqtext::decode_utf8(p.terms[0]), p.ignore_case.value_or(true), p.starts_with, d.alphabet, *d.regex_atoms);
}
static void probe_regex_part(const Index& idx, const RequestSearchPart& p, FuzzyTable& table) {
    if (!regex_device_enabled() || p.terms.empty()) return;
    const std::string key = fuzzy_key(p);
    if (table.count(key)) return;
    vqregex::Compiled c;
    try {
        c = regex_route(idx, p);
    } catch (const VelociError&) {
        return;  // the compiler reports it, request by request
    }
    if (!c.device) return;  // host route (regex_candidates)
    FuzzyProbe fp;
    fp.key = key;
    fp.path = p.path;
    if (!ends_with(fp.path, TEXTINDEX)) fp.path += TEXTINDEX;
    fp.regex = true;
    fp.dfa = std::move(c.dfa);
    table.emplace(key, std::move(fp));
}

// suggest_batch: a part with its own top whose top + skip fits k_dict_topn's buffer asks for a top-n probe (key: topn_key) when the device scores
// its hits and neither distance can reach the u8 cap (lower-cased term below 255 bytes, every term of the dictionary below 200: then the
// long-string branch of the scoring rule cannot occur either)
static void probe_part(const Index& idx, const RequestSearchPart& p, FuzzyTable& table, bool suggest_batch = false) {
    if (p.is_regex) return probe_regex_part(idx, p, table);
    if (!needs_dictionary_scan(p)) return;
    const std::string key = fuzzy_key(p);
    const size_t top_n = p.top.value_or(0) + p.skip.value_or(0);
    const bool ask_topn = suggest_batch && suggest_topn_enabled() && p.top && top_n >= *p.top && top_n >= 1 && top_n <= kTopnMax;
    if (table.count(ask_topn ? topn_key(p) : key)) return;
    FuzzyProbe fp;
    fp.key = key;
    fp.path = p.path;
    if (!ends_with(fp.path, TEXTINDEX)) fp.path += TEXTINDEX;
    auto dit = idx.dict.find(fp.path);
    if (dit == idx.dict.end()) return;  // the compiler reports FstNotFound
    // match-set automaton (search_field.rs:85-95): built from the ORIGINAL term
    fp.max_d = std::min<uint32_t>(clamped_lev(p), 4);
    fp.transposition = p.ignore_case.value_or(false);
    fp.ci = p.ignore_case.value_or(true);
    fp.prefix = p.starts_with;
    fp.lower_term = vqtext::to_lower_utf8(p.terms[0]);
    fp.lev = clamped_lev(p);
    fp.check_prefix = p.starts_with || fp.lev != 0;  // :302
    const auto cps = vqtext::decode_utf8(p.terms[0]);
    if (cps.size() >= kDictMaxPattern) {
        fp.status = ERR_UNSUPPORTED;
        fp.error = "fuzzy / prefix search with a term of " + std::to_string(cps.size()) + " characters (the dictionary scan takes fewer than " +
                   std::to_string(kDictMaxPattern) + ")";
    }
    for (uint32_t cp : cps) fp.query.push_back(fp.ci ? vqtext::lower_cp(cp) : cp);
    if (ask_topn && fp.status == 0 && fp.lower_term.size() < 255 && dit->second.max_term_bytes < 200 && probe_scored_on_device(idx, fp)) {
        fp.top_n = uint32_t(top_n);
        fp.key = topn_key(p);
        table.emplace(fp.key, std::move(fp));
        return;
    }
    if (!table.count(key)) table.emplace(key, std::move(fp));
}
static void probe_tree(const Index& idx, const SearchRequest& r, FuzzyTable& table) {
    if (r.kind == SearchRequest::Search) probe_part(idx, r.part, table);
    else
        for (auto& q : r.tree.queries) probe_tree(idx, q, table);
}
// score of every match of a probe (search_field.rs:304-321), shared by all requests of the batch that contain the leaf
void score_fuzzy_probe(const Index& idx, FuzzyProbe& fp) {
    if (fp.status != 0) return;
    const Dictionary& dict = idx.dict.at(fp.path);
    fp.scores.resize(fp.matches.size());
    for (size_t i = 0; i < fp.matches.size(); ++i) {
        const std::string lower_hit = vqtext::to_lower_utf8(dict.terms[fp.matches[i]]);
        const bool prefix_matches = fp.check_prefix && lower_hit.size() >= fp.lower_term.size() && lower_hit.compare(0, fp.lower_term.size(), fp.lower_term) == 0;
        fp.scores[i] = default_score_for_distance(scoring_distance(lower_hit, fp.lower_term, fp.lev), prefix_matches);
    }
}

void collect_suggest_probes(const Index& idx, const Request& req, FuzzyTable& table) {
    if (req.suggest)
        for (auto& p : *req.suggest) probe_part(idx, p, table);
}

void collect_suggest_batch_probes(const Index& idx, const Request& req, FuzzyTable& table) {
    if (req.suggest)
        for (auto& p : *req.suggest) probe_part(idx, p, table, true);
}

void collect_fuzzy_probes(const Index& idx, const Request& req, FuzzyTable& table) {
    if (req.search_req) probe_tree(idx, *req.search_req, table);
    if (req.filter) probe_tree(idx, *req.filter, table);
    if (req.phrase_boosts)
        for (auto& pb : *req.phrase_boosts) {
            probe_part(idx, pb.search1, table);
            probe_part(idx, pb.search2, table);
        }
    if (req.boost_term)
        for (auto& p : *req.boost_term) probe_part(idx, p, table);
}

}  // namespace vq
