// The dictionary side of a search part (term_lookup.cpp): which terms of a field's dictionary a RequestSearchPart matches and what they score,
// before any posting is read.  The query compiler asks per leaf (Compiler::field_result), suggest and highlight ask per part
// (text_requests.cpp).  The probe side — what the device must scan before lookup_terms can run, under the same keys — is declared in engine.hpp
// (fuzzy_key, topn_key, collect_*_probes, regex_route, score_fuzzy_probe): exec.cpp, prepass.cpp and capi.cpp call it.
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "engine.hpp"

namespace vq {

struct Leaf {  // PlanStepFieldSearchToTokenIds + its result (execution_plan.rs:16-44, plan_steps.rs:137-148)
    const vqreq::RequestSearchPart* part = nullptr;  // the request's own part (it outlives the compilation)
    std::string key;                          // part->key(), built once
    const PostingStore* store = nullptr;      // "<path>.to_anchor_id_score", looked up once
    std::string path;  // with ".textindex"
    bool get_scores = false, get_ids = false, store_term_id_hits = false;
    bool return_term = false, return_term_lowercase = false, store_term_texts = false;  // execution_plan.rs:16-44
    std::vector<std::pair<uint32_t, std::string>> terms;  // term id -> text (search_field.rs:347-353), ascending ids
    bool computed = false;
    std::vector<std::pair<uint32_t, float>> hits_scores;  // (term id, term score), ascending term id
    std::vector<uint32_t> hits_ids;                        // term ids
    std::map<uint32_t, ExplainRecs> explain;               // options.explain: the dictionary result's records per term id (search_field.rs:334-343)
};

inline bool part_explains(const vqreq::RequestSearchPart& p) { return p.options && p.options->explain; }  // search_request.rs:182-184

// get_term_ids_in_field (search_field.rs:277-398), dictionary side only: fills l.path, hits_scores / hits_ids, terms and explain from l.part.
// `fuzzy`: the batch's answered dictionary probes (fuzzy / prefix / regex leaves); topn_probes: it may hold top-n probes of a suggest batch.
void lookup_terms(const Index& idx, const FuzzyTable* fuzzy, bool topn_probes, Leaf& l, bool get_scores, bool get_ids);
// token_value (search_field.rs:391-395): the term-keyed boost column shapes l.hits_scores (and l.explain)
void apply_token_value(const Index& idx, const vqreq::RequestBoostPart& tv, Leaf& l);
// boost function, parameter, skip_when_score and score expression of a RequestBoostPart -> cb (the column's pointers are the caller's)
void fill_boost_params(DColBoost& cb, const vqreq::RequestBoostPart& b);

}  // namespace vq
