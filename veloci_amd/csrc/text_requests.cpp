// The requests that answer with texts, not with documents: suggest, highlight (snippets) and the why_found_info of finished searches.  Host
// work over the dictionary (term_lookup.cpp) and the host copies of the token / text stores; exec.cpp, prepass.cpp and capi.cpp call in
// (declarations: engine.hpp).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "compile_internal.hpp"
#include "term_lookup.hpp"
#include "text.hpp"

namespace vq {

using namespace vqreq;

// suggest (search_field.rs:194-219): one part's matched terms with lower-cased texts and scores — get_term_ids_in_field with get_scores,
// return_term and return_term_lowercase; the dictionary scan of a fuzzy / prefix part has run on the device (`fuzzy`).
std::vector<SuggestEntry> suggest_part(const Index& idx, const RequestSearchPart& part, const FuzzyTable* fuzzy, bool topn_probes) {
    Leaf l;
    l.part = &part;
    l.get_scores = true;
    l.return_term = true;
    l.return_term_lowercase = true;
    lookup_terms(idx, fuzzy, topn_probes, l, true, false);
    if (part.token_value) apply_token_value(idx, *part.token_value, l);
    std::vector<SuggestEntry> out;
    std::map<uint32_t, const std::string*> text;
    for (auto& t : l.terms) text[t.first] = &t.second;
    for (auto& h : l.hits_scores) out.push_back(SuggestEntry{*text.at(h.first), h.second, h.first});
    return out;
}


// highlight (search_field.rs:233-245): the texts that contain a matched token, each with its snippet (highlight_field.rs:187-272) and the
// best score among its matched tokens (resolve_token_hits_to_text_id with snippets, search_field.rs:550-639).  `part.terms` are already
// normalised; the dictionary scan of a fuzzy / prefix part has run on the device (`fuzzy`).  Host work over the host copies of
// tokens_to_text_id / text_id_to_token_ids: one text at a time, a few dozen tokens each.
namespace {
// the snippet of n tokens: is_hit(i) marks the tokens to tag, append(out, i) writes token i's text
template <class IsHit, class Append>
std::string snippet_of_tokens(size_t n, IsHit is_hit, Append append_text, const vqreq::SnippetInfo& opt, bool* any) {
    const int64_t around = opt.num_words_around_snippet * 2;  // token separator token separator
    // one walk: hits closer than `around` tokens share a window (group_hit_positions_for_snippet :19-37); a window reaches `around` tokens
    // to both sides of its hits (grouped_to_positions_for_snippet :39-43)
    std::string out;
    int64_t first_hit = -1, last_hit = -1, group_first = -1, group_last = -1;
    uint64_t windows = 0;
    auto close_group = [&]() {
        if (group_first < 0) return;
        if (windows < opt.max_snippets) {
            if (windows) out += opt.snippet_connector;
            const size_t lo = size_t(std::max<int64_t>(group_first - around, 0)), hi = size_t(std::min<int64_t>(group_last + around + 1, int64_t(n)));
            for (size_t i = lo; i < hi; ++i) {
                if (is_hit(i)) {
                    out += opt.snippet_start_tag;
                    append_text(out, i);
                    out += opt.snippet_end_tag;
                } else append_text(out, i);
            }
        }
        ++windows;
    };
    for (size_t i = 0; i < n; ++i) {
        if (!is_hit(i)) continue;
        if (first_hit < 0) first_hit = int64_t(i);
        if (group_first < 0 || int64_t(i) - group_last >= around) {
            close_group();
            group_first = int64_t(i);
        }
        group_last = last_hit = int64_t(i);
    }
    close_group();
    *any = first_hit >= 0;
    if (!*any) return out;
    if (first_hit > around) out.insert(0, opt.snippet_connector);             // ellipsis_snippet :73-90
    if (last_hit < int64_t(n) - around) out += opt.snippet_connector;
    return out;
}
std::string snippet_of_text(const Dictionary& dict, const uint32_t* toks, size_t n, const std::vector<uint32_t>& wanted_sorted, const vqreq::SnippetInfo& opt, bool* any) {
    return snippet_of_tokens(
        n, [&](size_t i) { return std::binary_search(wanted_sorted.begin(), wanted_sorted.end(), toks[i]); },
        [&](std::string& out, size_t i) {
            if (toks[i] < dict.terms.size()) out += dict.terms[toks[i]];
        },
        opt, any);
}
void check_snippet_window(const vqreq::SnippetInfo& opt) {
    if (opt.num_words_around_snippet < 0 || opt.num_words_around_snippet > 0x3FFFFFFF)  // the reference's window arithmetic overflows / panics there
        throw VelociError(ERR_INVALID_REQUEST, "InvalidRequest: \"snippet_info.num_words_around_snippet out of range\" ");
}
}  // namespace

// highlight_text (highlight_field.rs:92-146): `text` with the tokens that are in `terms` tagged — what why_found highlighting applies to every text
// of a returned document (highlight_on_original_document, :148-185) with the field's why_found_terms.  nullopt: nothing to highlight.
std::optional<std::string> highlight_text(const std::string& text, const std::vector<std::string>& terms, const vqreq::SnippetInfo& opt, bool tokenized) {
    check_snippet_window(opt);
    std::vector<std::string> set = terms;
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    if (set.size() == 1 && set[0] == text) return opt.snippet_start_tag + text + opt.snippet_end_tag;  // one hit that is the whole text
    if (!tokenized) return std::nullopt;
    const std::vector<vqtext::TokenSpan> tokens = vqtext::tokenize_grouped(text);
    std::vector<char> hit(tokens.size(), 0);
    for (size_t i = 0; i < tokens.size(); ++i) hit[i] = std::binary_search(set.begin(), set.end(), text.substr(tokens[i].begin, tokens[i].end - tokens[i].begin));
    bool any = false;
    std::string out = snippet_of_tokens(
        tokens.size(), [&](size_t i) { return hit[i] != 0; }, [&](std::string& o, size_t i) { o.append(text, tokens[i].begin, tokens[i].end - tokens[i].begin); }, opt, &any);
    // (contains_any_token is set while the windows are written: with max_snippets == 0 nothing is)
    if (!any || opt.max_snippets == 0) return std::nullopt;
    return out;
}

static const vqreq::SnippetInfo kDefaultSnippetInfo;
HighlightLookup highlight_lookup(const Index& idx, const RequestSearchPart& part, const FuzzyTable* fuzzy) {
    check_snippet_window(part.has_snippet_info ? part.snippet_info : kDefaultSnippetInfo);
    RequestSearchPart lookup = part;  // get_term_ids_in_field does not look at the snippet fields
    lookup.snippet.reset();
    lookup.has_snippet_info = false;
    Leaf l;
    l.part = &lookup;
    l.get_scores = true;
    lookup_terms(idx, fuzzy, false, l, true, false);
    if (lookup.token_value) apply_token_value(idx, *lookup.token_value, l);
    HighlightLookup lk;
    lk.path = l.path;
    lk.hits_scores = std::move(l.hits_scores);
    auto cit = idx.columns.find(lk.path.substr(0, lk.path.size() - std::strlen(TEXTINDEX)));
    lk.tokenized = cit != idx.columns.end() && cit->second.tokenize;
    lk.add_snippets = part.snippet.value_or(false);
    return lk;
}

bool highlight_snippet(const Index& idx, const HighlightLookup& lk, const RequestSearchPart& part, uint32_t text, const std::vector<uint32_t>& wanted_sorted, std::string* out) {
    const vqreq::SnippetInfo& opt = part.has_snippet_info ? part.snippet_info : kDefaultSnippetInfo;
    auto tit = idx.kv.find(lk.path + ".text_id_to_token_ids");
    if (tit == idx.kv.end()) throw VelociError(ERR_INDEX_NOT_FOUND, "Did not found path in indices " + lk.path + ".text_id_to_token_ids");
    const uint32_t *b, *e;
    if (!tit->second.host_row(text, &b, &e)) return false;
    bool any = false;
    *out = snippet_of_text(idx.dict.at(lk.path), b, size_t(e - b), wanted_sorted, opt, &any);
    return any;
}

std::vector<SuggestEntry> highlight_part(const Index& idx, const RequestSearchPart& part, const FuzzyTable* fuzzy) {
    return highlight_resolve(idx, part, highlight_lookup(idx, part, fuzzy));
}

std::vector<SuggestEntry> highlight_resolve(const Index& idx, const RequestSearchPart& part, const HighlightLookup& l) {
    const vqreq::SnippetInfo& opt = part.has_snippet_info ? part.snippet_info : kDefaultSnippetInfo;
    struct TextHit {
        uint32_t text;
        float score;
        uint32_t token, order;
    };
    std::vector<TextHit> hits;
    std::vector<std::pair<uint32_t, float>> ranked;  // (text id, best score): SearchFieldResult::hits_scores after the resolve step
    const std::string& path = l.path;
    const bool tokenized = l.tokenized;
    const bool add_snippets = l.add_snippets;
    std::map<uint32_t, std::string> snippets;
    for (auto& h : l.hits_scores) ranked.push_back(h);
    if (tokenized) {
        auto kit = idx.kv.find(path + TOKENS_TO_TEXT_ID);
        if (kit == idx.kv.end()) throw VelociError(ERR_INDEX_NOT_FOUND, "Did not found path in indices " + path + TOKENS_TO_TEXT_ID);
        uint32_t order = 0;
        for (auto& h : l.hits_scores) {
            const uint32_t *b, *e;
            if (!kit->second.host_row(h.first, &b, &e)) continue;
            for (const uint32_t* v = b; v != e; ++v) hits.push_back({*v, h.second, h.first, order++});
        }
        std::sort(hits.begin(), hits.end(), [](const TextHit& a, const TextHit& b) { return a.text != b.text ? a.text < b.text : a.order < b.order; });
        if (!hits.empty()) {
            if (add_snippets) ranked.clear();  // :608-610
            const KVStore* t2t = nullptr;
            const Dictionary& dict = idx.dict.at(path);
            std::vector<uint32_t> wanted;
            for (size_t i = 0; i < hits.size();) {
                size_t j = i;
                float best = hits[i].score;
                wanted.clear();
                for (; j < hits.size() && hits[j].text == hits[i].text; ++j) {
                    if (std::fabs(hits[j].score) >= std::fabs(best)) best = hits[j].score;  // Iterator::max_by_key keeps the last maximum
                    wanted.push_back(hits[j].token);
                }
                const uint32_t text = hits[i].text;
                ranked.push_back({text, best});
                if (add_snippets) {
                    if (!t2t) {
                        auto tit = idx.kv.find(path + ".text_id_to_token_ids");
                        if (tit == idx.kv.end()) throw VelociError(ERR_INDEX_NOT_FOUND, "Did not found path in indices " + path + ".text_id_to_token_ids");
                        t2t = &tit->second;
                    }
                    std::sort(wanted.begin(), wanted.end());
                    const uint32_t *b, *e;
                    if (t2t->host_row(text, &b, &e)) {
                        bool any = false;
                        std::string sn = snippet_of_text(dict, b, size_t(e - b), wanted, opt, &any);
                        if (any) snippets[text] = std::move(sn);
                    } else if (std::binary_search(wanted.begin(), wanted.end(), text))  // the text is its own only token: all of it (highlight_field.rs:198-203)
                        snippets[text] = opt.snippet_start_tag + (text < dict.terms.size() ? dict.terms[text] : std::string()) + opt.snippet_end_tag;
                }
                i = j;
            }
        }
    }
    std::vector<SuggestEntry> out;
    for (auto& r : ranked) {  // get_text_score_id_from_result(false, ..) search_field.rs:160-192: indexing `highlight` panics for a hit without a snippet
        auto it = snippets.find(r.first);
        if (it == snippets.end())
            throw VelociError(ERR_INVALID_REQUEST, "InvalidRequest: \"highlight: hit " + std::to_string(r.first) + " has no snippet (the reference panics)\" ");
        out.push_back(SuggestEntry{it->second, r.second, r.first});
    }
    return out;
}

// get_why_found (src/search/why_found.rs:11-50) for the finished requests that asked for why_found together with select: for every searched field
// and every returned anchor, the anchor's texts of the field (join_anchor_to_leaf, facet.rs:75-93) highlighted with all term ids the search matched
// there (highlight_document with DEFAULT_SNIPPETINFO, highlight_field.rs:187-272); a text without a hit leaves no entry.
void complete_why_found_requests(const Index& idx, std::vector<std::unique_ptr<Result>>& results, std::vector<int>& status, std::vector<std::string>& errors) {
    static const vqreq::SnippetInfo kDefault;
    for (size_t i = 0; i < results.size(); ++i) {
        if (status[i] != 0 || !results[i] || !results[i]->why_found_plan) continue;
        Result& R = *results[i];
        try {
            for (auto& [path, wanted] : *R.why_found_plan) {  // (wanted: sorted, unique)
                if (wanted.empty() || R.ids.empty()) continue;  // why_found.rs:29-31
                const std::string field_name = path.substr(0, path.size() - std::strlen(TEXTINDEX));
                const std::vector<std::string> steps = get_steps_to_anchor(field_name);
                auto store = [&](const std::string& name) -> const KVStore& {
                    auto it = idx.kv.find(name);
                    if (it == idx.kv.end()) throw VelociError(ERR_INDEX_NOT_FOUND, "Did not found path in indices " + name);
                    return it->second;
                };
                std::vector<const KVStore*> chain;
                for (auto& st : steps) chain.push_back(&store(st + PARENT_TO_VALUE_ID));
                const KVStore& t2t = store(steps.back() + ".text_id_to_token_ids");
                auto dit = idx.dict.find(steps.back());
                if (dit == idx.dict.end()) throw VelociError(ERR_INDEX_NOT_FOUND, "Did not found path in indices " + steps.back() + ".fst");
                const Dictionary& dict = dit->second;
                std::vector<uint32_t> level, next;
                for (uint32_t anchor : R.ids) {
                    level.assign(1, anchor);
                    for (const KVStore* st : chain) {
                        next.clear();
                        for (uint32_t id : level) {
                            const uint32_t *rb, *re;
                            if (st->host_row(id, &rb, &re)) next.insert(next.end(), rb, re);
                        }
                        level.swap(next);
                    }
                    for (uint32_t value_id : level) {
                        const uint32_t *b, *e;
                        if (t2t.host_row(value_id, &b, &e)) {
                            bool any = false;
                            std::string sn = snippet_of_text(dict, b, size_t(e - b), wanted, kDefault, &any);
                            if (any) R.why_found_info[anchor][field_name].push_back(std::move(sn));
                        } else if (std::binary_search(wanted.begin(), wanted.end(), value_id))  // the text is its own only token: all of it (highlight_field.rs:198-203)
                            R.why_found_info[anchor][field_name].push_back(kDefault.snippet_start_tag + (value_id < dict.terms.size() ? dict.terms[value_id] : std::string()) +
                                                                           kDefault.snippet_end_tag);
                    }
                }
            }
        } catch (const VelociError& e) {
            status[i] = e.code;
            errors[i] = e.what();
            results[i].reset();
        }
    }
}

}  // namespace vq
