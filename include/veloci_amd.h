/*
 * veloci_amd.h — C ABI of the MI355X-native veloci query-execution path.
 *
 * This is the drop-in boundary.  The reference exposes the path as
 *
 *     pub fn search(request: Request, persistence: &Persistence)
 *         -> Result<SearchResult, VelociError>              (src/search.rs:143)
 *
 * and has no FFI of its own; every entry point below states which reference
 * interface it replaces.  Plain pointers and sizes only: a Rust `extern "C"`
 * block, cgo or ctypes can bind it (INTEGRATION.md shows the Rust stub).
 *
 * Threading: a `vq_index` is immutable after `vq_index_build`; `vq_search*`
 * may be called from many host threads on one index (reference: `Persistence:
 * Sync`, src/persistence.rs:80-84).  Errors: every call returns `VQ_OK` or an
 * error code and leaves a message for `vq_last_error()` (thread local) that
 * reproduces the reference's `VelociError` rendering (src/error.rs:5-43).
 */
#ifndef VELOCI_AMD_H
#define VELOCI_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- errors */

enum {
    VQ_OK = 0,
    /* VelociError::InvalidRequest (src/error.rs:11) and the reference's panics on
       malformed plans (execution_plan.rs:220,408,437; plan_steps.rs:287) */
    VQ_ERR_INVALID_REQUEST = 1,
    /* VelociError::FstNotFound: "field does not exist {path} (fst not found)" (src/error.rs:35) */
    VQ_ERR_FST_NOT_FOUND = 2,
    /* VelociError::StringError("Did not found path in indices ...") (src/persistence.rs:454-458) */
    VQ_ERR_INDEX_NOT_FOUND = 3,
    /* request uses a feature outside the GPU hot path (the declined explain combinations, why_found_info on the flat / sharded entry points, the bounds of DESIGN.md §7 ...): never silently ignored */
    VQ_ERR_UNSUPPORTED = 4,
    /* HIP runtime failure / no device / extension missing */
    VQ_ERR_DEVICE = 5,
    VQ_ERR_INVALID_ARGUMENT = 6,
    /* serde_json parse failure of the request text (VelociError::JsonError) */
    VQ_ERR_JSON = 7
};

/* Message of the last failing call on this thread ("" if none). */
const char* vq_last_error(void);

/* ------------------------------------------------------- index (load side)
 *
 * Replaces `Persistence::load` + `PersistenceIndices` (src/persistence.rs:52-60,
 * 206-291, 393-410) at the *decoded array* level: the caller (a Rust shim walking
 * `persistence.indices`, or the synthetic generator) hands over every index as
 * plain CSR arrays under the reference's own index names
 * ("<field>.textindex.to_anchor_id_score", "...tokens_to_text_id", ...,
 * suffix constants src/persistence.rs:23-50).  Arrays are copied; the caller may
 * free them after the call returns.
 *
 * Sharding: an index holds the anchors (documents) in
 * [doc_lo, doc_hi).  Anchor-valued lists may be passed whole or pre-sliced —
 * the loader drops anchors outside the range.  Anchor-keyed stores take
 * `key_base`: the id of the first key in the arrays handed over.
 */
typedef struct vq_index_builder vq_index_builder;
typedef struct vq_index vq_index;

vq_index_builder* vq_index_builder_new(uint32_t num_anchors, uint32_t doc_lo, uint32_t doc_hi);
void vq_index_builder_free(vq_index_builder*);

/* Term dictionary of "<field>.textindex" — replaces `indices.fst[path]`
 * (src/persistence.rs:59; built at src/create/create_fulltext.rs:53-80).
 * Terms are UTF-8, bytewise sorted, ordinal == term id.  Any plane: the fuzzy / prefix scan (k_dict_scan) stages the code points as u16
 * when all of them are below U+10000 and as u32 otherwise; query terms of any length up to 2^20 - 1 code points. */
int vq_index_add_fst(vq_index_builder*, const char* path, uint32_t num_terms,
                     const uint8_t* term_bytes, const uint64_t* term_offsets /* [num_terms+1] */);

/* Posting lists "<field>.textindex.to_anchor_id_score" — replaces
 * `TokenToAnchorScore::get_score_iter` (src/persistence.rs:80-82,
 * src/indices/persistence_score/token_to_anchor_score_vint.rs:150-204).
 * Per token: anchors ascending & unique, integer scores as stored
 * (converted to f16 with RNE at load, as `f16::from_f32(score as f32)` :155).
 * `global_lens` (may be NULL) gives each list's length in the *unsharded* index;
 * needed only when the arrays are pre-sliced to a shard. */
int vq_index_add_token_to_anchor_score(vq_index_builder*, const char* path, uint32_t num_tokens,
                                       const uint64_t* offsets /* [num_tokens+1] */,
                                       const uint32_t* anchors, const uint32_t* scores,
                                       const uint64_t* global_lens);

/* Any `IndexIdToParent<Output=u32>` store (src/persistence.rs:142-181):
 * ".tokens_to_text_id", ".text_id_to_anchor", ".parent_to_value_id",
 * ".anchor_to_text_id", ".value_id_to_anchor", ".value_id_to_parent",
 * ".text_id_to_token_ids".  Key k (k = key_base + row) maps to
 * values[offsets[row] .. offsets[row+1]]. */
int vq_index_add_key_value_store(vq_index_builder*, const char* path, uint32_t key_base,
                                 uint32_t num_keys, const uint64_t* offsets, const uint32_t* values);

/* "<field>.textindex.phrase_pair_to_anchor" — replaces
 * `PhrasePairToAnchor::get_values((u32,u32))` (src/persistence.rs:84-87,
 * src/indices/persistence_data_binary_search.rs:167-202).  Keys sorted by (t1,t2). */
int vq_index_add_phrase_pair_to_anchor(vq_index_builder*, const char* path, uint64_t num_pairs,
                                       const uint32_t* t1, const uint32_t* t2,
                                       const uint64_t* offsets /* [num_pairs+1] */,
                                       const uint32_t* anchors);

/* "<field>.boost_valid_to_value" — replaces `persistence.get_boost(path)`
 * (src/persistence.rs boost_valueid_to_value; read at src/search/boost.rs:490-494).
 * `present[row]` != 0 when key (key_base+row) has a value; value_bits = f32 bits. */
int vq_index_add_boost(vq_index_builder*, const char* path, uint32_t key_base, uint32_t num_keys,
                       const uint8_t* present /* may be NULL = all present */,
                       const uint32_t* value_bits);

/* Column metadata consulted on the query path: `is_anchor_identity_column`
 * (src/search/search_field.rs:474-480, src/search/boost.rs:60-66) and
 * `textindex_metadata.options.tokenize` (src/search/search_field.rs:650-658). */
int vq_index_set_column_meta(vq_index_builder*, const char* field, int is_anchor_identity_column, int tokenize);

/* Stage everything into HBM on `device` (padded segmented arrays) and return the
 * immutable index.  The builder stays valid and must still be freed. */
int vq_index_build(vq_index_builder*, int device, vq_index** out);
void vq_index_free(vq_index*);

/* Run this index's launches on an existing HIP stream (hipStream_t as void*);
 * NULL restores the index's own stream. */
int vq_index_set_stream(vq_index*, void* hip_stream);
/* Two caller streams: the scans of vq_search_batch_partial run on `scan_stream`, everything vq_merge_partials* launches (shard merge,
 * facet selection, result download) on `finish_stream`, which waits for the batch's scan through an event.  A caller that pipelines
 * batches puts its collective on `finish_stream` too (after making that stream wait for the scan, e.g. an event recorded on
 * `scan_stream` right after vq_search_batch_partial returned): the gather and merge of batch c then overlap the scan of batch c+1. */
int vq_index_set_streams(vq_index*, void* scan_stream, void* finish_stream);
/* Sharded deployments: a few requests need numbers that are sums over all shards before they can be compiled (result sizes of AND
 * operands, lengths of merged leaf lists — set_op.rs:388-393 orders an AND's score sum by them).  `fn(ctx, values, n)` must replace
 * values[0..n) by their sums over all ranks (an all-reduce; every rank calls it with the same n, in the same order) and return 0.
 * Without it a shard declines such requests with VQ_ERR_UNSUPPORTED.  Called from inside vq_search_batch_partial. */
typedef int (*vq_allreduce_u64_fn)(void* ctx, uint64_t* values, size_t n);
int vq_index_set_allreduce(vq_index*, vq_allreduce_u64_fn fn, void* ctx);
/* Bytes of HBM held by the staged image. */
uint64_t vq_index_device_bytes(const vq_index*);

/* --------------------------------------------------------------- requests
 *
 * `vq_request` == `search::Request` (src/search/request/mod.rs:15-87), parsed
 * from its serde-JSON rendering.  Unknown keys are ignored (as serde does). */
typedef struct vq_request vq_request;

int vq_request_parse(const char* json, size_t len, vq_request** out);
/* A handle given to vq_search_batch_partial(_at) or vq_shard_step_begin may be freed as soon as the call returns, while the partial batch or
 * step is still alive: they share the parsed request with the handle.  Every other entry point is done with its requests when it returns. */
void vq_request_free(vq_request*);
/* What the parser understood: every field of search::Request (src/search/request/mod.rs:15-87, search_request.rs:6-179, boost_request.rs:4-33,
 * facet_request.rs:2-11) in declaration order, absent Options as null, `select` / `snippet_info` as "present" booleans, f32 values as their bit
 * patterns (u32).  Pinned by tests/golden/request_parse.json against an independent restatement of serde's rules.  Thread-local string. */
const char* vq_request_to_json(const vq_request*);
/* 1 when the request asks for facets (Request::facets, src/search/request/mod.rs:39, is a non-empty list), else 0: what decides whether a sharded
 * step exchanges histograms — taken from the PARSED request, the same on every rank. */
int vq_request_has_facets(const vq_request*);
/* str::to_lowercase as the dictionary side applies it (src/search/search_field.rs:284,312).  Returns the byte length written to `out`, or
 * (size_t)-1 when `cap` is too small.  Diagnostic: swept over every code point by tests/test_request_parse.py. */
size_t vq_debug_to_lowercase(const char* utf8, size_t len, char* out, size_t cap);
/* util::normalize_text (src/util.rs:11-29) as vq_highlight_json applies it to a part's terms; same conventions.  Diagnostic: compared with an
 * independent regex engine by tests/test_request_parse.py. */
size_t vq_debug_normalize_text(const char* utf8, size_t len, char* out, size_t cap);
/* The request compiler's id-list sort (value ids behind 1:n boost lists: ascending, duplicate-free, in place; returns the new length).  Diagnostic:
 * its three regimes are compared with an independent sort by tests/test_request_parse.py. */
size_t vq_debug_sort_unique_u32(uint32_t* ids, size_t n);
/* Compile a request against an index without launching anything (host-only): 0 = ready to scan, negative = a pre-pass would run first (-1 union /
 * locality jobs, -2 count pre-pass, -3 range jobs), otherwise the error code the search would return.  Diagnostic: the CPU sanitizer build (`make asan`) runs it over the
 * request fixtures; tools/compile_bench.py times it. */
int vq_debug_compile(const vq_index*, const vq_request*);
/* The route of a regex part (a RequestSearchPart as JSON with is_regex): 0 and the sizes of its DFA when the dictionary is scanned on the
 * device (k_dict_regex); VQ_ERR_UNSUPPORTED with the reason in vq_last_error() when the part stays on the host route (structure outside the
 * DFA compiler, a table beyond the kernel's LDS budget, VQ_NO_REGEX_DEVICE=1); the search's own error for a part that cannot run at all.
 * `states` / `classes` may be null. */
int vq_debug_regex_compile(const vq_index*, const char* part_json, size_t len, uint32_t* states, uint32_t* classes);

/* --------------------------------------------------------------- doc sets
 *
 * A set of anchor ids staged in HBM and attached to requests: the request then behaves exactly as if its `filter` were one leaf whose hits_ids are
 * the set's ids (a leaf with a label of its own), and-ed with the request's own `filter` when it has one.  Nothing else about the request
 * changes: vq_request_to_json prints the same text, no JSON key exists for it.  A doc set is immutable; any number of requests and threads may
 * share one.  It belongs to the index it was made for: a search that pairs it with another index answers VQ_ERR_INVALID_ARGUMENT for that request. */
typedef struct vq_docset vq_docset;
/* ids: n u32 anchor ids, any order, duplicates allowed; ids_on_device != 0: `ids` is device memory on the index's GPU (4-byte aligned, complete before
 * the call).  VQ_ERR_INVALID_ARGUMENT when an id is >= the index's number of anchors (the count is in vq_last_error).  Synchronous. */
int vq_docset_create(const vq_index*, const uint32_t* ids, uint64_t n, int ids_on_device, vq_docset** out);
/* The set a filter tree selects, evaluated once on the device.  filter_json: a SearchRequest tree, exactly what Request.filter holds (a leaf, or
 * and / or over trees).  within: NULL, or a set of the same index that is and-ed in.  The ids are exactly those the filter of a request with `filter`
 * = this tree and doc set = `within` selects, so a search with the resulting set attached answers bit for bit what the same search answers with the
 * tree as its `filter`.  Every decline and error is the one that search returns (unknown path, more than 64 lists, a filter that reduces to
 * nothing, ...); VQ_ERR_JSON for text that does not parse, VQ_ERR_INVALID_ARGUMENT for a `within` of another index.  On a shard the set's length is
 * the sum over the shards: one u64 goes through the hook of vq_index_set_allreduce (every rank calls in the same order); without the hook a shard
 * answers VQ_ERR_UNSUPPORTED.  The result is an ordinary doc set, also as the `within` of another call.  Synchronous. */
int vq_docset_from_filter(const vq_index*, const char* filter_json, size_t len, const vq_docset* within, vq_docset** out);
/* Set algebra over staged sets of one index, on the device.  AND / OR: n >= 1 operands (n == 1: a set equal to the operand).  MINUS: n >= 1,
 * sets[0] without the ids of any of sets[1 .. n).  NOT: n == 1, every anchor of the index's doc range that is not in the set (never an id >= the
 * number of anchors).  n has no upper bound.  The result is an ordinary, immutable doc set: attached to a request, as `within`, as an operand of
 * another combine.  Synchronous; any number of threads may call concurrently, also on shared operands, which are only read and may be freed right
 * after the call.  Two routes fill the result's bitmap: the word route folds the operands' bitmap words; the probe route — an AND with at least one
 * operand that carries no bitmap, a MINUS whose minuend carries none — streams the smallest such operand's ids and tests each against the others,
 * so its cost follows the small set.  VQ_NO_SETOP_PROBE=1 in the environment (read at every call) sends everything through the word route.
 * VQ_ERR_INVALID_ARGUMENT for n == 0, a null operand, an unknown op, NOT with n != 1, an operand made for another index.  On a shard the
 * result's length is the sum over the shards: one u64 goes through the hook of vq_index_set_allreduce (every rank calls in the same order); without
 * the hook a shard answers VQ_ERR_UNSUPPORTED.  An unsharded index never calls the hook. */
enum { VQ_DOCSET_AND = 0, VQ_DOCSET_OR = 1, VQ_DOCSET_MINUS = 2, VQ_DOCSET_NOT = 3 };
int vq_docset_combine(const vq_index*, int op, const vq_docset* const* sets, size_t n, vq_docset** out);
/* The set of the docs whose numeric column values satisfy every clause, selected on the device.  ranges_json: a non-empty list of clauses,
 *   [{"field": "price", "gte": 10, "lt": 100}, {"field": "rating", "missing": true, "gt": 4.5}, {"field": "tags[].rank", "lte": 3}]
 * `field` names the column "<field>.boost_valid_to_value", resolved as a request's boosts resolve it.  At most one of gt / gte and one of lt / lte
 * (a null bound counts as absent).  A present, non-NaN f32 value v satisfies `gte: b` exactly when (double)v >= b, b being the f64 the JSON number
 * parses to, and likewise for the others: `lte: 0.1` does not select a stored float32(0.1), `gte: 0.1` does.  -0 equals +0, the infinities and the
 * denormals are ordinary values, NaN satisfies no clause and counts as present.  A clause without bounds selects every present non-NaN value, a
 * lower bound above the upper one nothing.  `missing` (default false): whether a doc without a value satisfies the clause.  A field without "[]":
 * the column is keyed by doc, as a boost reads it (no value below key_base, behind the last key, or with the presence bit clear).  A field with
 * "[]": the column is keyed by value id, a value belongs to the anchor in the first entry of its "<field>.value_id_to_anchor" row; the clause holds
 * for a doc when any of its present values is inside the interval, with `missing` also when it has no present value.  Any number of clauses, also
 * on one field; OR and NOT are vq_docset_combine's.  within: NULL, or a set of the same index that is and-ed in.  Two routes fill the result's
 * bitmap: the stream route reads the columns over the doc range; the probe route — `within` carries no bitmap and no clause is 1:n — gathers the
 * values of within's ids, so its cost follows the small set.  VQ_NO_RANGE_PROBE=1 in the environment (read at every call) sends everything through
 * the stream route.  VQ_ERR_JSON for text that does not parse or a value of the wrong type (a bound that is not a number); VQ_ERR_INVALID_ARGUMENT
 * for an empty list, a clause without `field`, gt with gte, lt with lte, an unknown key, a ".token_values" column (keyed by term ids), a `within`
 * of another index; the search's VQ_ERR_INDEX_NOT_FOUND ("Did not found path in indices ...") for an unknown column or a 1:n field without its
 * value_id_to_anchor store.  The result is an ordinary, immutable doc set.  Synchronous; any number of threads may call concurrently.  On a shard
 * the set's length is the sum over the shards: one u64 goes through the hook of vq_index_set_allreduce (every rank calls in the same order);
 * without the hook a shard answers VQ_ERR_UNSUPPORTED.  An unsharded index never calls the hook. */
int vq_docset_from_ranges(const vq_index*, const char* ranges_json, size_t len, const vq_docset* within, vq_docset** out);
/* self-check (tests): -1 for a set not made from ranges, 0 when the stream route built it, 1 when the probe route did */
int vq_debug_docset_range_route(const vq_docset*);
/* The set's ids inside this index's doc range — sorted, unique, unpadded — to `out`: host memory, or with out_on_device != 0 device memory on the
 * index's GPU (4-byte aligned; copied device to device on the library's stream, finished when the call returns; the index must still exist).  At
 * most `cap` ids are copied; returns the local length (0 with the reason in vq_last_error when the copy failed). */
uint64_t vq_docset_ids(const vq_docset*, uint32_t* out, uint64_t cap, int out_on_device);
/* self-check (tests): -1 for a set no combine made, 0 when the word route built it, 1 when the probe route did */
int vq_debug_docset_route(const vq_docset*);
uint64_t vq_docset_len(const vq_docset*);        /* unique ids of the whole set (the same on every shard) */
uint64_t vq_docset_local_len(const vq_docset*);  /* those inside this index's doc range */
uint64_t vq_docset_device_bytes(const vq_docset*);
/* self-check (tests): part 0 = the local ids without padding, 1 = bitmap words, 2 = rank_dir, 3 = tile_dir, 4 = the local ids with their padding to
 * a multiple of 4 entries; returns the element count (0: the set carries no such part), copies min(count, cap) elements */
uint64_t vq_debug_docset_part(const vq_docset*, int part, uint32_t* out, uint64_t cap);
/* measurement: with VQ_DOCSET_TIMING=1 in the environment a set records the HIP event times (ms) of its construction — marking the ids (a set from a filter: evaluating
 * the filter's program), counting and scanning, expanding; 0, or -1 when the set recorded none */
int vq_debug_docset_timings(const vq_docset*, float* ms_mark, float* ms_count_scan, float* ms_expand);
void vq_docset_free(vq_docset*);
/* attaches the set to the request (NULL detaches).  The request keeps the set alive: freeing the handle afterwards is allowed.  A partial batch
 * or step in flight that was made from the request is not affected: it keeps the set the request had when the batch was made. */
int vq_request_set_docset(vq_request*, const vq_docset*);

/* ---------------------------------------------------------------- results
 *
 * `vq_result` == `search::SearchResult` (src/search/result/search_result.rs:9-26). */
typedef struct vq_result vq_result;

uint64_t vq_result_num_hits(const vq_result*);
uint64_t vq_result_execution_time_ns(const vq_result*);
size_t vq_result_len(const vq_result*);            /* data.len() */
const uint32_t* vq_result_ids(const vq_result*);   /* data[i].id    */
const float* vq_result_scores(const vq_result*);   /* data[i].score */
size_t vq_result_num_facets(const vq_result*);
const char* vq_result_facet_field(const vq_result*, size_t facet);
size_t vq_result_facet_len(const vq_result*, size_t facet);
const char* vq_result_facet_value(const vq_result*, size_t facet, size_t i);
uint64_t vq_result_facet_count(const vq_result*, size_t facet, size_t i);
/* serde_json rendering of the SearchResult (ids/scores/facets/why_found_terms/why_found_info), for diffing. */
const char* vq_result_to_json(const vq_result*);
/* The facet counts of a staged set: facets_json is what Request.facets holds ([{"field": .., "top": ..}, ...]).
 * *out is an ordinary vq_result: num_hits = vq_docset_len, no hits, the facets as a search over exactly these docs reports them.
 * The set's docs are counted on the device (one kernel for all fields, no scoring, no candidate pool); `top` up to 1024 is ranked there, `top: null`
 * over more values and larger tops on the host: count descending, value id ascending, zero counts dropped.  Fields come back in request order, the
 * same field twice gives two entries; a value id beyond the dictionary renders as "".  An empty set yields every field with an empty list, an empty
 * (or null) facet list a result without facets.  Unknown fields, a missing dictionary and facet sources that are not staged decline exactly as a
 * search with these facets does; VQ_ERR_JSON for text that does not parse, VQ_ERR_INVALID_ARGUMENT for a null argument or a set of another index.
 * Synchronous; any number of threads may call concurrently, also on one set, which is only read.  VQ_NO_DOCSET_FACET_LDS=1 in the environment
 * (read at every call) counts short histograms like long ones (through the counter cache instead of a whole histogram in LDS).  On a shard the
 * local histograms are summed over the shards before ranking: one call of the hook of vq_index_set_allreduce with every field's counters as u64
 * (every rank calls in the same order; none when the whole set is empty); without the hook a shard answers VQ_ERR_UNSUPPORTED.  An unsharded
 * index never calls the hook. */
int vq_docset_facets(const vq_index*, const vq_docset*, const char* facets_json, size_t len, vq_result** out);
/* measurement: with VQ_DOCSET_TIMING=1 in the environment, the HIP event time (ms) of the count kernel of this thread's last vq_docset_facets;
 * negative when none was launched or timed */
float vq_debug_docset_facets_count_ms(void);
/* Numeric aggregations of a staged set, computed on the device: the counterpart of vq_docset_facets for the numeric columns.  aggs_json: a
 * non-empty list of {"field": "price"} or {"field": "price", "edges": [0, 10, 100]}; results come back in request order, the same field may occur
 * twice.  `field` names the column "<field>.boost_valid_to_value", resolved exactly as vq_docset_from_ranges resolves it, with its errors.
 * A field without "[]" (keyed by doc): a doc of the set without a value (below key_base, behind the last key, presence bit clear) counts in
 * `missing`, a NaN in `nan`, everything else — the infinities included — in `count`, min, max, sum and its bucket; docs = vq_docset_len =
 * missing + nan + count.  A field with "[]" (keyed by value id): a present value belongs to the anchor in the first entry of its
 * "<field>.value_id_to_anchor" row (empty rows and later entries count for nothing); every present value whose anchor is in the set is
 * aggregated, count + nan is their number, `missing` the number of docs of the set with no present value.  min / max: compared by value (-0 equals
 * +0 and a zero is reported as +0.0); both 0 when count == 0.  sum: the exact sum of the finite counted values rounded once to f64, ties to even
 * — bit-identical across runs, atomic orders and shardings; +inf when only positive infinities occur besides, -inf when only negative ones, NaN
 * with both; 0.0 when nothing is counted.  edges: at most 1023 strictly ascending numbers; n_buckets = edges + 1 (0 and buckets NULL without
 * `edges`): bucket 0 counts v < e0, bucket i e(i-1) <= v < e(i), the last v >= e(last), a stored f32 compared as f64 against the edge as written
 * (the rule of vq_docset_from_ranges); two edges between two neighbouring f32 values leave the bucket between them empty.  The buckets add up to
 * count, and for a column keyed by doc bucket i equals the length of the set and-ed with vq_docset_from_ranges' {gte: e(i-1), lt: e(i)} (a 1:n
 * column counts values, a doc set docs).  VQ_ERR_JSON for text that does not
 * parse or a value of the wrong type (an edge that is not a number); VQ_ERR_INVALID_ARGUMENT for a null argument, an empty list, an aggregation
 * without `field`, an unknown key, more than 1023 edges, edges that do not strictly ascend, a ".token_values" column, a set of another index;
 * the search's VQ_ERR_INDEX_NOT_FOUND for an unknown column or a 1:n field without its value_id_to_anchor store.  Synchronous; any number of
 * threads may call concurrently, also on one set, which is only read.  VQ_NO_AGG_PREREDUCE=1 in the environment (read at every call) adds every
 * value to the sum with atomics of its own instead of summing a wave's values first (same result); VQ_AGG_MAX_GRID=<n> (read at every call;
 * tests) caps the workgroups per aggregation.  On a shard every rank ends with the whole
 * set's answer: counters, buckets and the sum's limbs go through the hook of vq_index_set_allreduce in one call, min and max are agreed in four
 * more; every rank calls in the same order, none when the whole set is empty; without the hook a shard answers
 * VQ_ERR_UNSUPPORTED.  An unsharded index never calls the hook. */
typedef struct vq_docset_aggs vq_docset_aggs;
typedef struct vq_docset_agg {
    uint64_t docs, count, missing, nan;
    double sum;
    float min, max;
    uint64_t n_buckets;
    const uint64_t* buckets; /* owned by the vq_docset_aggs */
} vq_docset_agg;
int vq_docset_aggregate(const vq_index*, const vq_docset*, const char* aggs_json, size_t len, vq_docset_aggs** out);
size_t vq_docset_aggs_len(const vq_docset_aggs*);
const vq_docset_agg* vq_docset_aggs_get(const vq_docset_aggs*, size_t i); /* NULL beyond the list */
void vq_docset_aggs_free(vq_docset_aggs*);
/* measurement: with VQ_DOCSET_TIMING=1 in the environment, the HIP event time (ms) of the kernels of this thread's last vq_docset_aggregate;
 * negative when none was launched or timed */
float vq_debug_docset_aggregate_ms(void);
/* A staged set ordered by a numeric column: rows [skip, skip + top) of the set's docs, selected on the device without a search and without a host
 * copy of the column.  spec_json: {"field": "price", "top": 10, "skip": 0, "descending": false, "with_missing": true} (all but `field` optional,
 * with these defaults).  `field` names the column "<field>.boost_valid_to_value", resolved exactly as vq_docset_from_ranges and
 * vq_docset_aggregate resolve it, with their errors.  Every doc of the set gets one 32-bit sort key: a doc with a number the order-preserving key
 * of its f32 (ascending) or that key's complement (descending) — -0 and +0 share a key, the infinities are numbers; a doc whose value is NaN
 * 0xFFFFFFFE in both directions; a doc without a value (below key_base, behind the last key, presence bit clear) 0xFFFFFFFF.  The order is sort key
 * ascending, then doc id ascending: in both directions numbers, then NaN docs, then missing docs, ties always by ascending doc id.  A field with
 * "[]" (keyed by value id, joined through "<field>.value_id_to_anchor", first entry of the row, as the aggregations read it): a doc's key is the
 * smallest sort key among its present values — its minimum when ascending, its maximum when descending —, the NaN key when all its present values
 * are NaN, the missing key when it has none.  with_missing false lists only docs with a number; a page past them is short or empty.  The rows:
 * vq_docset_top_len of them, vq_docset_top_docs / _values / _kinds in row order (owned by the handle): kind 0 a number, 1 NaN, 2 missing; value
 * the f32 recovered from the key (a zero is +0.0), NaN for kind 1, 0.0 for kind 2.  vq_docset_top_counters writes docs, count, nan, missing (in
 * docs of the set, docs = count + nan + missing; for a column keyed by doc the numbers of vq_docset_aggregate).  The result is a pure function of
 * the inputs: two calls give identical rows, nothing depends on the order of atomics.  top + skip <= 65536 (the search's bound on ranked hits):
 * above it VQ_ERR_UNSUPPORTED; top = 0 returns counters and no rows.  VQ_ERR_JSON for text that does not parse or a value of the wrong type;
 * VQ_ERR_INVALID_ARGUMENT for a null argument, a spec without `field`, an unknown key, a negative or fractional top / skip, a ".token_values"
 * column, a set of another index; the search's VQ_ERR_INDEX_NOT_FOUND for an unknown column or a 1:n field without its value_id_to_anchor store.
 * Synchronous; any number of threads may call concurrently, also on one set, which is only read; a call owns its scratch: 4 bytes per local id,
 * and for a field with "[]" 4 bytes per doc of the index's doc range.  VQ_TOP_MAX_GRID=<n> (read at every call; tests) caps the workgroups of every
 * kernel, VQ_TOP_FORCE_SELECT=1 (read at every call; tests) runs the select even when the set holds no more than top + skip docs.
 * Shards: a top-k is no sum, so no hook is called.  On a sharded index the call returns the shard's part: its own first top + skip rows with skip
 * not applied, its local counters (docs = the set's docs inside the shard), vq_docset_top_is_partial 1.  vq_docset_top_merge (host only) merges
 * the parts of all shards by (sort key, doc), applies skip and top and sums the counters; VQ_ERR_INVALID_ARGUMENT for no part, a null part, or
 * parts whose top, skip, direction, with_missing or field differ.  vq_docset_top_pack writes a part's flat byte image (a fixed 64-byte header,
 * the field, the rows as (sort key, doc) pairs) to out when cap suffices and returns the bytes needed (0: an error), so that ranks in different
 * processes can all-gather it; vq_docset_top_unpack validates every length, the counters and the order of the rows and answers
 * VQ_ERR_INVALID_ARGUMENT for a malformed image. */
typedef struct vq_docset_top vq_docset_top;
int vq_docset_top_by(const vq_index*, const vq_docset*, const char* spec_json, size_t len, vq_docset_top** out);
size_t vq_docset_top_len(const vq_docset_top*);
const uint32_t* vq_docset_top_docs(const vq_docset_top*);
const float* vq_docset_top_values(const vq_docset_top*);
const uint8_t* vq_docset_top_kinds(const vq_docset_top*);
void vq_docset_top_counters(const vq_docset_top*, uint64_t* out4); /* docs, count, nan, missing */
int vq_docset_top_is_partial(const vq_docset_top*);
int vq_docset_top_merge(const vq_docset_top* const* parts, size_t n, vq_docset_top** out);
size_t vq_docset_top_pack(const vq_docset_top*, uint8_t* out, size_t cap);
int vq_docset_top_unpack(const uint8_t* bytes, size_t len, vq_docset_top** out);
void vq_docset_top_free(vq_docset_top*);
/* measurement: with VQ_DOCSET_TIMING=1 in the environment, the HIP event time (ms) of the kernels of this thread's last vq_docset_top_by;
 * negative when none was launched or timed */
float vq_debug_docset_top_ms(void);
/* `SearchResult.why_found_terms` (src/search/result/search_result.rs:21-25, filled at src/search.rs:186 when the request says
 * `why_found: true`): per text index path the matched dictionary terms, as JSON {"<path>": ["term", ...]} (thread-local string;
 * the reference's map and list orders are unspecified). */
const char* vq_result_why_found_terms_json(const vq_result*);
/* `SearchResult.why_found_info` (src/search.rs:220-224 = get_why_found, src/search/why_found.rs:11-50; what to_documents hands out per hit when
 * the request has a `select`, search.rs:83-88): for `why_found: true` together with `select`, per returned anchor and searched field the
 * anchor's texts of the field that hold a matched token, highlighted like vq_highlight_json's snippets with the default snippet options — as JSON
 * {"<anchor id>": {"<field>": ["text with <b>hits</b>", ...]}} (thread-local string); "null" when the request did not ask.  `select` itself is not
 * looked at, as in search::search: reading the selected fields is to_documents' work on the caller's document store.  Host work on the final
 * window of hits (needs the fields' `.parent_to_value_id` and `.text_id_to_token_ids` stores); vq_search / vq_search_json / vq_search_batch
 * only — the flat and the sharded entry points answer VQ_ERR_UNSUPPORTED for such a request. */
const char* vq_result_why_found_info_json(const vq_result*);
/* `explain: true` (src/search/request/mod.rs:83-86; or `options.explain` on the single leaf of a request): the `Explain` records
 * (src/search/result/explain.rs:2-21) of the returned hits, i.e. `SearchResult.explain.get(&hit.id)` of src/search.rs:86,96 — a JSON array
 * parallel to the hits, each element null or the hit's records in serde's form ({"TermToAnchor":{"term_score":..,"anchor_score":..,
 * "final_score":..,"term_id":..}}, {"LevenshteinScore":{"score":..,"text_or_token_id":"..","term_id":..}}, {"OrSumOverDistinctTerms":..},
 * {"Boost":..}; floats printed with %.9g).  "null" when the request did not ask.  The scores inside the records are recomputed on the
 * device for the returned hits only (k_explain).  Declined: explain together with phrase_boosts or a 1:n boost, explain on some leaves
 * only, and explain on the flat / sharded paths.  Thread-local string. */
const char* vq_result_explain_json(const vq_result*);
void vq_result_free(vq_result*);

/* ---------------------------------------------------------------- suggest
 *
 * == search_field::suggest_multi(persistence, request) (src/search/search_field.rs:194-219) when `json` is a Request with
 * "suggest": [RequestSearchPart, ...] (+ top / skip), == search_field::suggest(persistence, &part) (:221-231) when it is a bare
 * RequestSearchPart.  Dictionary side only: the matched terms of every part (fuzzy / prefix scans run on the device, regex leaves on
 * the host), lower-cased texts, equal texts merged keeping the best score, ranked by score.  SuggestFieldResult = Vec<(String, Score, TermId)>. */
typedef struct vq_suggest_result vq_suggest_result;
int vq_suggest_json(const vq_index*, const char* json, size_t len, vq_suggest_result** out);
size_t vq_suggest_len(const vq_suggest_result*);
const char* vq_suggest_text(const vq_suggest_result*, size_t i);
float vq_suggest_score(const vq_suggest_result*, size_t i);
uint32_t vq_suggest_term_id(const vq_suggest_result*, size_t i);
void vq_suggest_free(vq_suggest_result*);
/* n independent suggest requests (each text as vq_suggest_json takes it: a Request with "suggest" parts, or a bare RequestSearchPart)
 * answered as one device batch.  out[i] receives request i's result, or NULL with status[i] != VQ_OK; the text of the first failing
 * request is in vq_last_error.  Returns VQ_OK when the batch ran.  Every out[i] equals what vq_suggest_json returns for json[i].
 * The dictionary scans of all requests run together (equal probes once).  A part with its own `top` whose top + skip is at most 1848 has
 * the reference's top-n loop run on the device (k_dict_topn) and only that loop's final buffer copied back; VQ_NO_SUGGEST_TOPN=1 keeps
 * every part on the route that copies all matches back. */
int vq_suggest_batch(const vq_index*, const char* const* json, const size_t* len, size_t n, vq_suggest_result** out, int* status);

/* ---------------------------------------------------------------- highlight
 * == search_field::highlight(persistence, &mut part) (src/search/search_field.rs:233-245): `json` is a bare RequestSearchPart with
 * "snippet": true (+ optional "snippet_info", src/search/request/snippet_info.rs).  The terms are normalised (util::normalize_text), matched
 * against the field's dictionary (prefix / fuzzy scans run on the device), resolved to the texts that contain a matched token
 * (resolve_token_hits_to_text_id, :550-639) and every such text is returned as a snippet (highlight_document, src/highlight_field.rs:187-272)
 * with the best score among its matched tokens, ranked by score, cut by the part's top / skip.  Entry i: vq_suggest_text = the snippet,
 * vq_suggest_score, vq_suggest_term_id = the text id.  Where the reference panics (a hit without a snippet: an untokenised field, "snippet" not
 * set) the call returns VQ_ERR_INVALID_REQUEST.  Needs the field's tokens_to_text_id and text_id_to_token_ids stores. */
int vq_highlight_json(const vq_index*, const char* json, size_t len, vq_suggest_result** out);
/* n independent highlight parts (each text as vq_highlight_json takes it) answered as one device batch.  out[i] receives part i's result, or
 * NULL with status[i] != VQ_OK; the text of the first failing part is in vq_last_error.  Returns VQ_OK when the batch ran.  Every out[i] equals
 * what vq_highlight_json returns for json[i].  The dictionary scans of all parts run together (equal probes once).  A part with "snippet": true
 * and its own `top` (1 <= top + skip <= 1024) on a tokenized field, whose token scores are all finite and above 0, has its texts ranked on the
 * device: the best matched-token score per text (k_text_best) and the page's top + skip texts by (score descending, text id ascending)
 * (k_text_select) — only those texts get a snippet.  That needs the field's tokens_to_text_id and text_id_to_token_ids to hold the same
 * (token, text) pairs, checked once per field on first use (a tokens_to_text_id table the index build did not stage goes to HBM then); any other
 * part is answered inside the batch by vq_highlight_json's own code.  VQ_NO_HIGHLIGHT_RANK=1 keeps every part on that route. */
int vq_highlight_batch(const vq_index*, const char* const* json, const size_t* len, size_t n, vq_suggest_result** out, int* status);
/* == highlight_field::highlight_text(text, set, opt, tokenizer) (src/highlight_field.rs:92-146): `text` with the tokens that are in `terms` wrapped in
 * the snippet tags, cut into windows like vq_highlight_json's snippets — what why_found highlighting (highlight_on_original_document, :148-185) applies to
 * every text of a returned document with the field's terms from vq_result_why_found_terms_json.  `tokenized` = the field has a tokenizer (the default
 * separators of src/tokenizer/mod.rs:21-23); `snippet_info_json` may be NULL (DEFAULT_SNIPPETINFO); term_lens may be NULL (C strings).  Returns the
 * snippet's byte length — the bytes are in `out` when the length fits `cap`, otherwise call again with a larger buffer —, VQ_HIGHLIGHT_NONE when
 * nothing is highlighted (the reference's None), VQ_HIGHLIGHT_ERROR on an error (vq_last_error).  Host work; needs no index. */
#define VQ_HIGHLIGHT_NONE ((size_t)-1)
#define VQ_HIGHLIGHT_ERROR ((size_t)-2)
size_t vq_highlight_text(const char* text, size_t len, const char* const* terms, const size_t* term_lens, size_t n_terms, const char* snippet_info_json,
                         size_t json_len, int tokenized, char* out, size_t cap);

/* ----------------------------------------------------------------- search */

/* == search::search(request, &persistence) (src/search.rs:143-228). */
int vq_search(const vq_index*, const vq_request*, vq_result** out);
/* Same, from the request's JSON text. */
int vq_search_json(const vq_index*, const char* json, size_t len, vq_result** out);
/* Throughput path: n independent searches executed as one device batch
 * (the reference's equivalent is n concurrent `search()` calls from server
 * threads, server/rocket_server.rs:139-145).  out[i] receives request i's
 * result, or NULL with status[i] != VQ_OK.  Returns VQ_OK when the batch ran. */
int vq_search_batch(const vq_index*, const vq_request* const* requests, size_t n,
                    vq_result** out, int* status);

/* Same batch, flat output without per-result objects (facets are not reported through this entry):
 * request i's hits go to ids/scores[i * stride .. i * stride + counts[i]).  `stride` must be >= the
 * largest `top` of the batch. */
int vq_search_batch_flat(const vq_index*, const vq_request* const* requests, size_t n, size_t stride,
                         uint64_t* num_hits /* [n] */, uint32_t* counts /* [n] */,
                         uint32_t* ids /* [n*stride] */, float* scores /* [n*stride] */, int* status /* [n] */);

/* ------------------------------------------------- shard-partial interface
 *
 * New surface (the reference has no sharding): a shard returns
 * its exact local top-(top+skip) with global doc ids, its local hit count and
 * its facet histograms over value ids; `vq_merge_partials` turns the gathered
 * partials of all shards into the final results.  The gather itself is done by
 * the caller (RCCL all-gather of the packed buffers). */
typedef struct vq_partial_batch vq_partial_batch;

/* The batch keeps the requests it was made from alive (a merge may run one again): the handles in `requests` may be freed, or given another
 * doc set (vq_request_set_docset: the batch keeps the set it was made with), as soon as the call returns.  The same holds for
 * vq_search_batch_partial_at. */
int vq_search_batch_partial(const vq_index*, const vq_request* const* requests, size_t n,
                            vq_partial_batch** out);
/* Packed, fixed-size representation of the partials (same size on every shard
 * for the same requests).  Resident in HBM: `device_ptr` can be handed to RCCL. */
size_t vq_partial_bytes(const vq_partial_batch*);
void* vq_partial_device_ptr(vq_partial_batch*);
/* The batch's facet histograms (u32 counts over value ids; 0 bytes without facet requests) live behind the all-gathered part
 * and are NOT part of it: the caller sums them over the shards in place with an all-reduce (ncclSum on `vq_partial_hist_bytes / 4`
 * u32 — SURVEY.md 8e: facet counts are additive) before `vq_merge_partials*`.  With one shard nothing needs to be done. */
size_t vq_partial_hist_bytes(const vq_partial_batch*);
void* vq_partial_hist_device_ptr(vq_partial_batch*);
/* Merge `num_shards` gathered packed buffers (device memory, shard-major,
 * each `vq_partial_bytes` long) into final results; facet counts are read from `local`'s (already summed) histograms. */
int vq_merge_partials(const vq_index*, vq_partial_batch* local, const void* gathered_device,
                      uint32_t num_shards, vq_result** out, int* status);
/* One scan ranks the best 1024 hits of a request.  A request whose top + skip reaches further (the reference has no limit: src/search/sort.rs:5-22,
 * src/search.rs:230-239) comes back from vq_merge_partials as its PAGE 0 — all 1024 ranked hits, top / skip not applied yet — with
 * vq_result_is_page() == 1.  The caller (every rank alike: the merged page is the same on all of them) sends vq_request_page_after(request, score and
 * id of the page's last hit) through partial -> all-gather -> merge again, appends the hits, and repeats while a page comes back full; then it
 * applies skip / top (apply_top_skip).  vq_search / vq_search_batch do this themselves on an unsharded index; the flat merges decline such requests. */
int vq_result_is_page(const vq_result*);
int vq_request_page_after(const vq_request*, float score, uint32_t id, vq_request** out);
/* Same merge with flat output (see vq_search_batch_flat). */
int vq_merge_partials_flat(const vq_index*, vq_partial_batch* local, const void* gathered_device, uint32_t num_shards, size_t stride,
                           uint64_t* num_hits, uint32_t* counts, uint32_t* ids, float* scores, int* status);
/* One collective per step while the step still runs as a pipeline of chunks (the host compiles chunk c+1 while the GPU scans chunk c):
 * every chunk is searched with `vq_search_batch_partial_at` into its own workspace `slot` (0 .. vq_partial_slots()-1) with its partial placed at
 * `arena_offset` of the index's partial arena (`vq_index_partial_arena_ptr`; offsets are multiples of 256, chunk c+1 starts at
 * arena_offset_c + round_up(vq_partial_total_bytes(chunk c), 256); VQ_ERR_UNSUPPORTED when the arena — 64 MiB — is too small).  The caller
 * all-gathers the arena's used prefix [0, S) ONCE, then merges every chunk with `vq_merge_partials_flat_strided(gathered + arena_offset_c,
 * num_shards, shard_stride = S)`.  Chunks with facet histograms still need their all-reduce (vq_partial_hist_*), so a caller would keep such
 * steps on the per-chunk path. */
int vq_search_batch_partial_at(const vq_index*, const vq_request* const* requests, size_t n, int slot, size_t arena_offset, vq_partial_batch** out);
int vq_partial_slots(void);
void* vq_index_partial_arena_ptr(const vq_index*);
size_t vq_partial_total_bytes(const vq_partial_batch*);
int vq_merge_partials_flat_strided(const vq_index*, vq_partial_batch* local, const void* gathered_device, uint32_t num_shards, size_t shard_stride,
                                   size_t stride, uint64_t* num_hits, uint32_t* counts, uint32_t* ids, float* scores, int* status);
void vq_partial_free(vq_partial_batch*);

/* ---- the sharded step inside the library (no counterpart in the reference, which does not shard).
 * One communicator per index / rank: rank 0 takes a unique id (`vq_comm_unique_id`, VQ_COMM_ID_BYTES bytes), hands it to the other ranks
 * by whatever means the host program has, every rank calls `vq_comm_init` (ncclCommInitRank on the index's device; RCCL is loaded at run
 * time).  From then on `vq_shard_step_flat` is one whole step on this rank: compile -> scans -> RCCL all-gather of the packed partials
 * (hit counts + top-k keys of every query; every rank must pass the SAME requests) and all-reduce of the facet histograms -> merge ->
 * one download; the communicator also serves the sums over the shards that some requests need before compilation (what
 * `vq_index_set_allreduce` asks a caller for).  `vq_shard_step_begin` returns as soon as the step's work is queued, `vq_shard_step_end`
 * delivers it: a caller that begins step i+1 before it ends step i keeps two steps in flight (the scans of one overlap the exchange and
 * merge of the other; at most two).  Results are those of `vq_search_batch_flat` on the unsharded index, bit for bit; requests whose
 * top + skip exceeds 1024 are declined here when the step has an exchange (page them through vq_merge_partials); an index that answers alone pages them itself.  On an index without a communicator the step is the same
 * pipeline without an exchange: begin / end then keep two batches in flight on an unsharded index.
 * `vq_comm_init_custom` takes the exchange from the caller instead (all-gather of `bytes_per_rank` bytes per rank into a rank-major
 * buffer; in-place sum of u32 counters — both on device memory, to be ordered on `hip_stream` or finished before they return): several
 * shards inside one process, tests.
 * The handles passed to `vq_shard_step_begin` may be freed, or given another doc set, as soon as the call returns: the step keeps the requests,
 * and the doc sets, it was begun with until it is ended or freed. */
#define VQ_COMM_ID_BYTES 128
typedef struct vq_shard_step vq_shard_step;
typedef int (*vq_allgather_fn)(void* ctx, const void* local_device, void* gathered_device, size_t bytes_per_rank, void* hip_stream);
typedef int (*vq_allreduce_u32_fn)(void* ctx, void* inout_device, size_t count, void* hip_stream);
int vq_comm_unique_id(void* id_out);
int vq_comm_init(vq_index*, int nranks, int rank, const void* unique_id);
int vq_comm_init_custom(vq_index*, int nranks, int rank, vq_allgather_fn allgather, vq_allreduce_u32_fn allreduce_u32, void* ctx);
int vq_comm_destroy(vq_index*);
int vq_shard_step_begin(const vq_index*, const vq_request* const* requests, size_t n, vq_shard_step** out);
int vq_shard_step_end(vq_shard_step*, size_t stride, uint64_t* num_hits, uint32_t* counts, uint32_t* ids, float* scores, int* status); /* frees the step */
void vq_shard_step_free(vq_shard_step*); /* a step that is given up instead of ended */
int vq_shard_step_flat(const vq_index*, const vq_request* const* requests, size_t n, size_t stride, uint64_t* num_hits, uint32_t* counts,
                       uint32_t* ids, float* scores, int* status);

/* ------------------------------------------------------------ measurement */

/* Device time (ms, HIP events on the index's stream) and launch count of the
 * dominant scan kernel accumulated since the last call with reset != 0. */
int vq_profile_read(const vq_index*, int reset, double* scan_kernel_ms, uint64_t* scan_launches,
                    uint64_t* algorithmic_bytes);
/* Enable (1) / disable (0) the HIP-event bracketing used by vq_profile_read / vq_profile_json. */
int vq_profile_enable(vq_index*, int on);
/* Per-kernel accounting since the last reset, as JSON (thread-local string, valid until the next call on this thread):
 * {"batches": n, "kernels": {"<kernel>": {"ms", "launches", "layout_bytes", "algorithmic_bytes", "queries", "scan"}}}.
 * ms = device time between HIP events recorded around the launch on its stream; layout_bytes = the bytes THIS data layout has to
 * move for those launches (bitmap words of dense lists, 4 B per id of scattered lists, 6 B per streamed posting, the bytes of
 * per-hit gathers as counted by the kernels, 8 B per key written) — the roofline numerator; algorithmic_bytes = SURVEY.md 8(d)'s
 * posting-streaming accounting, kept for comparison. */
const char* vq_profile_json(const vq_index*, int reset);

/* ------------------------------------------------------------- self-checks (tests) */

/* Number of f16 inputs for which the kernels' fast `a / 100.0f` differs from the correctly rounded division (must be 0);
 * 0xFFFFFFFF when no device is available. */
uint32_t vq_debug_div100_mismatches(void);

/* The column boost of the scans (add_boost, boost.rs:470-504: skip_when_score, the row of the doc, boost function, expression) alone, one lane
 * per element, through the very device functions the scan kernels call: out_scores[i] = the boost applied to scores[i] for doc docs[i];
 * out_log10_factor[i] = the f32 log10(value + param) an explain record carries for a Log10 boost, for every doc with a present row whatever the
 * function and the skip rule, 0.0f for a doc without one.  fun: -1 none, 0 Log2, 1 Log10, 2 Multiply, 3 Add, 4 Replace; `expression` (or NULL)
 * and the n_skip (0 .. 4) `skip` values are parsed as a request's `expression` / `skip_when_score`.  The column covers docs key_base .. key_base
 * + num_keys - 1: `values` holds num_keys f32, `present_words` (or NULL: every row present) (num_keys + 31) / 32 words, bit r & 31 of word r >> 5
 * set for a present row r.  n in 1 .. 2^24, num_keys at most 2^24.  0; -1 without a device; -2 for arguments outside these ranges or a boost
 * the request parser refuses (vq_last_error says which). */
int vq_debug_col_boost(int fun, float param, const char* expression, const float* skip, uint32_t n_skip, const float* values, uint32_t num_keys,
                       const uint32_t* present_words, uint32_t key_base, const uint32_t* docs, const float* scores, uint32_t n, float* out_scores,
                       float* out_log10_factor);

/* Requests of this index that were run a second time on the exact kernels because the short cut of a speculative one could not be confirmed:
 * an OR of the shape k_scan_probe_or takes ranks only the docs that hold its rarest term and is confirmed by the k-th key it returns. */
uint64_t vq_index_speculative_reruns(const vq_index*);
/* Totals of this index's vq_suggest_batch calls since it was built: probes answered by k_dict_topn, and match records copied back from the
 * device (a top-n probe counts min(its matches, top + skip + 200) entries, every other probe its matches).  Either pointer may be NULL. */
void vq_index_suggest_topn_probes(const vq_index*, uint64_t* topn_probes, uint64_t* records_copied_back);
/* k_dict_topn (the top-n loop of search_field.rs:322-333 + sort.rs:25-34) on one crafted stream: n (term, class) pairs in term-id order, class =
 * 2 * distance + prefix_matches (< 512), top_n in 1 .. 1848.  Writes the loop's final buffer in buffer order (the out arrays take top_n + 200
 * entries) and its length.  0; -1 without a device; -2 for arguments outside these ranges. */
int vq_debug_dict_topn(const uint32_t* terms, const uint32_t* classes, uint32_t n, uint32_t top_n, uint32_t* out_terms, uint32_t* out_classes, uint32_t* out_n);

/* Totals of this index's vq_highlight_batch calls since it was built: parts whose texts were ranked and cut to the page on the device
 * (k_text_best / k_text_select), and snippets the batch entry point built on the host (a device part builds one per returned text, a part on
 * the host route one per text that holds a matched token).  Either pointer may be NULL. */
void vq_index_highlight_rank_counts(const vq_index*, uint64_t* device_parts, uint64_t* snippets_built);
/* k_text_best + k_text_select on a caller's CSR: row r = row_vals[row_off[r] .. row_off[r + 1]) holds text ids below num_texts and carries the
 * f32 score bits row_score_bits[r] (finite, > 0); top_n in 1 .. 1024.  Writes the top_n texts by (best score descending, text id ascending) —
 * the out arrays take top_n entries —, their number and the number of texts that occur in any row.  0; -1 without a device; -2 for arguments
 * outside these ranges. */
int vq_debug_text_rank(const uint64_t* row_off, const uint32_t* row_vals, const uint32_t* row_score_bits, uint32_t num_rows, uint32_t num_texts, uint32_t top_n,
                       uint32_t* out_texts, uint32_t* out_score_bits, uint32_t* out_n, uint32_t* out_touched);

/* The facet selection kernels (k_facet_select / k_facet_select_wide: facet.rs:19-23, count descending; ties by value id ascending) on a
 * caller's histogram of `num_values` counts, placed `misalign` (0-3) counters behind a 16-byte boundary as inside a batch's histogram area:
 * writes the best min(top, non-zero counts) entries, returns their number, -1 on failure. */
int vq_debug_facet_select(const uint32_t* hist, uint32_t num_values, uint32_t top, uint32_t misalign, uint32_t* out_values, uint32_t* out_counts);

/* ---- the two merges every search ends in, alone on crafted key tables (tests/test_gpu_merge_kernels.py).  A key is
 * (order-preserving f32 score bits << 32) | doc id, 0 = an empty slot; n_jobs >= 1 jobs with top_k[j] in 1 .. 1024 share ONE launch, job j's
 * output at the exclusive prefix of top_k.  0; -1 on a device error; -2 — before the device is touched — for a null pointer, n_jobs,
 * num_shards or an n_spans of 0, a top_k outside 1 .. 1024, more than 2^24 keys in all, a stride_pad that is no multiple of 8 (or above 2^20). */
/* k_merge_spans.  Job j: n_spans[j] spans of top_k[j] keys, back to back in span_keys (as the scans leave them: a set per span, zeros behind
 * it).  out_keys: sum(top_k) keys — job j's best top_k[j], sorted descending, zeros behind. */
int vq_debug_merge_spans(const uint64_t* span_keys, const uint32_t* n_spans, const uint32_t* top_k, uint32_t n_jobs, uint64_t* out_keys);
/* k_finalize.  num_shards partial buffers in the layout a batch uses (hits[n_jobs], counters[n_jobs], keys[sum(top_k)]; no histograms),
 * `stride_pad` extra bytes between them (the strided merge of a chunked step).  shard_keys: shard-major, per shard the jobs' keys at the prefix
 * of top_k; shard_hits: shard-major, one u64 per job.  out_ids / out_score_bits (f32 bit patterns): sum(top_k) entries, job j's ranked window at
 * the prefix of top_k, out_n[j] of them real; out_hits[j]: the shards' hit counts summed. */
int vq_debug_finalize(const uint64_t* shard_keys, const uint64_t* shard_hits, uint32_t num_shards, size_t stride_pad, const uint32_t* top_k, uint32_t n_jobs,
                      uint32_t* out_ids, uint32_t* out_score_bits, uint32_t* out_n, uint64_t* out_hits);

/* ---- the pre-pass drivers alone (prepass.cpp run_union_jobs / run_locality_jobs / run_range_jobs / run_boost1n_jobs): what a batch runs before its
 * scans, on jobs the caller describes the way the request compiler does, with every list the drivers build copied back whole.  Jobs are passed as a
 * CSR: job j owns ids[job_off[j] .. job_off[j + 1]) (job_off[0] == 0, at most 2^31 ids, n_jobs >= 1) and names its stores by the paths they were
 * loaded under.  Lists come back to back in out_docs / out_val_bits (f32 bit patterns), `out_cap` entries each: job j's out_len[j] entries and the
 * 8 sentinel entries (0xFFFFFFFF, 0.0f) behind them start at the sum of out_len[i] + 8 over i < j.  Every function returns 0; -1 without a device or
 * when the driver fails; -2 for arguments outside the ranges given here (a null pointer, an unknown path, a store without the device image the
 * driver reads, an id table that is no CSR, `out_cap` too small for the lists).  With profiling on (vq_profile_enable) the launches are
 * accounted in vq_profile_json like a batch's. */
/* K2, the union of posting lists with the per-doc maximum of term_score * (f16 score / 100): job j merges the lists `tokens` (ids below the
 * store's token count, at least one) of store_paths[j] ("<field>.textindex.to_anchor_id_score") with the term scores term_score_bits (f32 bits,
 * one per token).  route 0: the shipped rule (more than VQ_UNION_DENSE_MIN lists, 4096 by default, take the dense route of union_dense.hip);
 * 1: k_union for every job (one level up to 64 lists, two levels up to 4096; more is -2); 2: the dense route for every job.  out_max_bits[j]: the
 * largest value of job j's list, 0.0f for an empty one. */
int vq_debug_union_lists(const vq_index*, const char* const* store_paths, const uint64_t* job_off, const uint32_t* tokens, const uint32_t* term_score_bits,
                         uint32_t n_jobs, int route, uint64_t out_cap, uint32_t* out_len, uint32_t* out_max_bits, uint32_t* out_docs, uint32_t* out_val_bits);
/* K7, text locality of a field whose text ids are not anchors: job j gathers the rows of `tokens` (multiplicity kept; ids outside the table are
 * skipped) from t2t_paths[j] ("<field>.textindex.tokens_to_text_id" of a column that is not an anchor identity column) and expands the texts that
 * occur c > 1 times through t2a_paths[j] ("<field>.textindex.text_id_to_anchor") to (anchor, 2 * c * c), the smallest value per anchor, ascending
 * anchors of this shard.  When no job of the call gathers any entry nothing is launched: every out_len is 0 and the out arrays are left alone. */
int vq_debug_locality_lists(const vq_index*, const char* const* t2t_paths, const char* const* t2a_paths, const uint64_t* job_off, const uint32_t* tokens,
                            uint32_t n_jobs, uint64_t out_cap, uint32_t* out_len, uint32_t* out_docs, uint32_t* out_val_bits);
/* k_range_hits: job j counts the postings of the lists `tokens` (token_off CSR; ids below the token count; none, one — a lane per anchor — or
 * several — a workgroup per anchor) of store_paths[j] around its anchors (anchor_off CSR; strictly ascending, below 0xFFFFFFFF).  out_counts takes
 * 2 * anchor_off[n_jobs] numbers: [2k] the postings at anchor k, [2k + 1] those strictly between the job's previous anchor and anchor k (0 for a job's
 * first).  A sharded index needs vq_index_set_allreduce (the driver sums over the shards), else -2. */
int vq_debug_range_hits(const vq_index*, const char* const* store_paths, const uint64_t* token_off, const uint32_t* tokens, const uint64_t* anchor_off,
                        const uint32_t* anchors, uint32_t n_jobs, uint64_t* out_counts);
/* K10, a 1:n boost list: job j gathers the value ids of `text_ids` (ids outside the table are skipped) from to_parent_paths[j]
 * ("<leaf>.textindex.value_id_to_parent"), sorts them and maps every one that has a boost value in boost_paths[j] ("<boost>.boost_valid_to_value")
 * and a non-empty row in to_anchor_paths[j] ("<boost>.value_id_to_anchor") to (first anchor of the row, boost value), in value-id order.  The list
 * holds the pairs of this shard's anchors (out_len[j]); out_total[j] counts the pairs of all shards; out_flags[j]: bit 0 = the anchors never
 * decrease in value-id order, bit 1 = some anchor equals its predecessor. */
int vq_debug_boost1n_lists(const vq_index*, const char* const* to_parent_paths, const char* const* to_anchor_paths, const char* const* boost_paths,
                           const uint64_t* job_off, const uint32_t* text_ids, uint32_t n_jobs, uint64_t out_cap, uint32_t* out_len, uint32_t* out_total,
                           uint32_t* out_flags, uint32_t* out_docs, uint32_t* out_val_bits);
/* The count pre-pass alone (k_tile_scan in count mode): the n requests (doc sets attached or not; n >= 1) go through the compilation passes of a
 * batch up to and including the count pre-pass — dictionary scans and union / locality / range jobs first where a leaf needs them — and no result
 * scan is launched.  Per request: status[i] = VQ_OK when it was counted, VQ_COUNTS_NONE when it needs no count pre-pass, otherwise the error code
 * its search would return (the first such text is in vq_last_error; a null request: VQ_ERR_INVALID_ARGUMENT); has_filter[i] (0 / 1) and
 * filter_count[i], the ids of the filter (the request's `filter` and-ed with its doc set); n_spans[i] / tile_words[i], what the count query was
 * compiled with (0 for a request that was not counted).  The measured nodes of request i are entries node_off[i] .. node_off[i + 1] of node_ids
 * (the compiler's preorder number of the node inside search_req: the root is 0, an operand follows its predecessor's whole sub-tree), hits and
 * hits_in_filter, `out_cap` entries each; node_off takes n + 1 numbers.  hits_in_filter is 0 for a request without a filter (that counter is
 * never written).  summed == 0: the numbers of this shard as the kernel wrote them; 1: after the
 * sum over the shards (vq_index_set_allreduce), what the compiler goes by — the same on an unsharded index.  Returns 0; -1 without a device or
 * when a pre-pass fails; -2 for a null pointer, n == 0, summed outside 0 / 1 or `out_cap` too small for the nodes.  With profiling on the launch
 * is accounted under "k_tile_scan<count pre-pass>" like a batch's. */
#define VQ_COUNTS_NONE (-1)
int vq_debug_node_counts(const vq_index*, const vq_request* const* requests, size_t n, int summed, uint64_t out_cap, int* status, uint32_t* has_filter,
                         uint64_t* filter_count, uint32_t* n_spans, uint32_t* tile_words, uint64_t* node_off, uint32_t* node_ids, uint64_t* hits,
                         uint64_t* hits_in_filter);

const char* vq_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VELOCI_AMD_H */
