// Host-callable launchers of kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "device_types.hpp"

namespace vq {

struct DictProbe {  // one fuzzy / prefix scan of a dictionary (k_dict_scan)
    uint32_t m, max_d, flags, lm;  // flags: 1 transposition costs one, 2 prefix (starts_with); lm: code points of `lquery`, or 0xFFFFFFFF
    uint16_t query[64];            // match side: the ORIGINAL term (lower-cased per code point when case-insensitive)
    uint16_t lquery[64];           // scoring side: the lower-cased term (search_field.rs:298-300); lm == 0xFFFFFFFF: the host scores the matches
};
struct DictProbeW {  // one scan of k_dict_scan_wide: the query's code points as u32 in a side pool (any length, any plane)
    uint32_t m, max_d, flags, lm;  // as DictProbe (m < kDictMaxPattern)
    uint32_t q_off;                // pool[q_off, + m): match side
    uint32_t lq_off;               // pool[lq_off, + lm): scoring side (lm <= 64), unless lm == 0xFFFFFFFF
    uint32_t pad[2];
};
constexpr uint32_t kDictMaxPattern = 1u << 20;  // code points of a query term the wide scan takes (the packed descriptor's field)
struct DictMatch {  // one matched dictionary term, with what its score needs (search_field.rs:304-321, 691-732)
    uint32_t probe, term;
    uint32_t info;  // optimal-string-alignment distance of the lower-cased hit to the lower-cased term | plain Levenshtein distance << 8 (both
                    // capped at 255) | (lower-cased hit starts with the lower-cased term) << 16
};

struct UList {  // one input list of a union task (k_union)
    const uint32_t* docs;
    const void* scores;  // f16 anchor scores, or f32 values when flags & 1 (output of an earlier level)
    uint32_t len;
    float term_score;
    uint32_t flags, pad;
};
struct RangeJobD {  // k_range_hits: the leaf's lists [list_begin, + n_lists), its 1:n boost list's entry anchors [anchor_begin, + n_anchors) and the
                    // job's first block (n_lists == 1: 64 anchors per block, else one)
    uint32_t list_begin, n_lists, anchor_begin, n_anchors, block_begin, pad;
};
struct UTask {  // <= 64 lists merged by one wave per span
    uint32_t list_begin, n_lists;  // into the UList table
    uint32_t span_begin, n_spans;  // global span index of span 0; spans split the doc space at quantiles of list `pivot`
    uint32_t pivot, pad;           // absolute UList index of the longest list
};

struct FacetJob {
    uint32_t hist_off, num_values, top, out_off;
};

size_t tile_scan_lds_bytes(uint32_t n_bitmaps, uint32_t n_lists, uint32_t tile_words, uint32_t stack_depth, uint32_t cand_cap, uint32_t desc_cap, bool queue, uint32_t ml);

void launch_tile_scan(hipStream_t st, uint32_t total_spans, size_t lds_bytes, const uint8_t* blobs, const uint32_t* blob_off, const uint32_t* span_base,
                      const uint32_t* qmap, uint32_t nq, uint32_t stack_depth, uint32_t cand_cap, uint32_t desc_cap, unsigned long long* span_keys, unsigned long long* num_hits, uint32_t* hist, bool queue, uint32_t ml,
                      bool facet_cache = false);
void launch_scan_leaf_f32(hipStream_t st, uint32_t total_spans, const uint8_t* blobs, const uint32_t* blob_off, const uint32_t* span_base, const uint32_t* qmap,
                          uint32_t nq, uint32_t cand_cap, unsigned long long* span_keys, unsigned long long* num_hits, uint32_t* hist);
size_t scan_simple_lds_bytes(uint32_t cand_cap, uint32_t nv, uint32_t n_scatter, bool facet_cache);
uint32_t debug_div100_mismatches();
int debug_col_boost(DColBoost cb, const float* values, uint32_t num_keys, const uint32_t* present_words, uint32_t key_base, const uint32_t* docs, const float* scores,
                    uint32_t n, float* out_scores, float* out_log10_factor);
int debug_facet_select(const uint32_t* hist_host, uint32_t num_values, uint32_t top, uint32_t misalign, uint32_t* out_vals_host, uint32_t* out_counts_host);
void launch_scan_simple(hipStream_t st, bool wide, uint32_t n_scatter, uint32_t total_spans, const uint8_t* blobs, const uint32_t* blob_off, const uint32_t* span_base,
                        const uint32_t* qmap, uint32_t nq, uint32_t cand_cap, unsigned long long* span_keys, unsigned long long* num_hits, uint32_t* hist, bool facet_cache = false);
// k_scan_probe_* (scan_probe.hip): one kernel per shape class, each launched over a (span_base, qmap) table of its own
enum : uint32_t { kProbeAnd1 = 0, kProbeAnd2A0, kProbeAnd2A1, kProbeAnd2A2, kProbeAnd3A0, kProbeAnd3A1, kProbeAnd3A2, kProbeAnd3A3, kProbeOr, kProbeShapes };  // AND of ND operands beside the cover (ND >= 2: per number of array operands) / OR
size_t scan_probe_lds_bytes(uint32_t cand_cap, uint32_t nd, uint32_t na, uint32_t arr_slot);
uint32_t debug_probe_occupancy(uint32_t shape, size_t lds_bytes);
void launch_scan_probe_shape(hipStream_t st, uint32_t shape, uint32_t na_seen, uint32_t arr_slot, uint32_t total_spans, const uint8_t* blobs, const uint32_t* blob_off,
                             const uint32_t* span_base, const uint32_t* qmap, uint32_t nq, uint32_t cand_cap, unsigned long long* span_keys, unsigned long long* num_hits);
size_t scan_wide_lds_bytes(uint32_t cand_cap, uint32_t n_leaves, uint32_t n_scatter);
void launch_scan_wide(hipStream_t st, uint32_t max_leaves, uint32_t max_scatter, uint32_t total_spans, const uint8_t* blobs, const uint32_t* blob_off, const uint32_t* span_base,
                      const uint32_t* qmap, uint32_t nq, uint32_t cand_cap, unsigned long long* span_keys, unsigned long long* num_hits);
void launch_merge_spans(hipStream_t st, uint32_t nq, const uint8_t* blobs, const uint32_t* blob_off, const unsigned long long* span_keys,
                        unsigned long long* part_keys);
void launch_finalize(hipStream_t st, uint32_t nq, const uint8_t* blobs, const uint32_t* blob_off, const uint8_t* gathered, uint32_t num_shards,
                     size_t shard_stride, const PartialLayout& lay, uint32_t* res_ids, float* res_scores, uint32_t* res_n, unsigned long long* res_hits);
void launch_facet_select(hipStream_t st, uint32_t n_jobs, const FacetJob* jobs, const uint32_t* hist, uint32_t* out_vals, uint32_t* out_counts,
                         uint32_t* out_n);

void launch_range_hits(hipStream_t st, uint32_t n_blocks, uint32_t n_jobs, const UList* ulists, const RangeJobD* jobs, const uint32_t* anchors, unsigned long long* counts);
void launch_union(hipStream_t st, bool write, uint32_t total_spans, const UList* ulists, const UTask* tasks, const uint32_t* span_task, uint32_t* span_cnt,
                  const uint64_t* span_off, uint32_t* out_docs, float* out_vals, uint32_t* task_min);
// ---- dense union (union_dense.hip): leaves with more lists than two levels of k_union take
constexpr uint32_t kDenseBlockDocs = 2048;  // slab words per workgroup of the count / write passes; a job's slab is padded to whole blocks
struct UDenseList {  // one non-empty posting list of a group of jobs; lists[n] closes the table (first == the group's postings)
    const uint32_t* docs;
    const uint16_t* scores;
    uint64_t first;  // index of the list's first posting in the group's flattened order
    float term_score;
    uint32_t job;    // of the group
};
struct UDenseJob {
    uint64_t slab_off;             // first word of the job's slab
    uint64_t out_off;              // first entry of the job's list in the output arrays
    uint32_t block_begin, n_blocks;  // count / write workgroups: the group's first block of this job, blocks of the job (>= 1)
    uint32_t result, pad;          // index into the batch's UDenseResult table
};
struct UDenseResult {
    uint32_t len, max_key;  // entries written; largest order_f32(value), 0 = the list is empty
};
void launch_union_dense_scatter(hipStream_t st, const UDenseList* lists, uint32_t n_lists, uint64_t total_postings, const UDenseJob* jobs, uint32_t* slab, uint32_t lo_doc,
                                uint32_t range);
// count pass + prefix sums: block_cnt[b] becomes the entries of the job before block b (block_max: n_blocks words of scratch), results[] are set
void launch_union_dense_count(hipStream_t st, const UDenseJob* jobs, uint32_t n_jobs, uint32_t n_blocks, const uint32_t* slab, uint32_t* block_cnt, uint32_t* block_max,
                              UDenseResult* results);
void launch_union_dense_write(hipStream_t st, const UDenseJob* jobs, uint32_t n_jobs, uint32_t n_blocks, const uint32_t* slab, const uint32_t* block_off, uint32_t lo_doc,
                              uint32_t* out_docs, float* out_vals);
void launch_scan_union(hipStream_t st, bool with_or, uint32_t total_spans, const uint8_t* blobs, const uint32_t* blob_off, const uint32_t* span_base, const uint32_t* qmap,
                       uint32_t nq, uint32_t cand_cap, unsigned long long* span_keys, unsigned long long* num_hits);
// all n_probes scan the SAME dictionary image (off / chars); matches are appended to out[0 .. out_cap) (the count keeps running beyond the cap)
void launch_dict_scan(hipStream_t st, const DictProbe* d_probes, uint32_t probe_base, uint32_t n_probes, const uint32_t* off, const uint16_t* chars, const uint16_t* low_chars,
                      uint32_t num_terms, uint32_t* out_count, uint32_t out_cap, DictMatch* out);
// the same over a 16-bit (char_bytes 2) or 32-bit (char_bytes 4) image, with the probes' queries in `pool`
void launch_dict_scan_wide(hipStream_t st, uint32_t char_bytes, const DictProbeW* d_probes, const uint32_t* pool, uint32_t probe_base, uint32_t n_probes, const uint32_t* off,
                           const void* chars, const void* low_chars, uint32_t num_terms, uint32_t* out_count, uint32_t out_cap, DictMatch* out);
// ---- regex leaves (dict_regex.hip): the probe's DFA (regex_dfa.hpp) in the kernel's format.  Its tables are u16 words of a pool, at
// [tab_off, + regex_words16): next[states * classes] with the states premultiplied by the number of classes, the class of every code point
// below 128, the class of the k-th non-ASCII code point of the dictionary's alphabet; tab_off is a multiple of 8 (16-byte loads).
struct RegexProbeD {
    uint32_t tab_off, n_next;      // n_next = states * classes (< 65536)
    uint32_t start, first_accept;  // premultiplied: the walk starts at `start`, a term matches when it ends at or above `first_accept`
};
__host__ __device__ inline uint32_t regex_words16(uint32_t n_next, uint32_t n_alpha) { return (n_next + 128u + n_alpha + 7u) & ~7u; }
// n_probes probes (d_probes[0 ..), numbered from probe_base in the output) over ONE dictionary: its offsets, its RAW image, the non-ASCII part
// of its alphabet.  small_tables: every probe's tables fit vqregex::kLdsTableBytesSmall.  Output as launch_dict_scan (info = 0).
void launch_dict_regex(hipStream_t st, uint32_t char_bytes, bool small_tables, const RegexProbeD* d_probes, const uint16_t* pool, const uint32_t* alpha, uint32_t n_alpha,
                       uint32_t probe_base, uint32_t n_probes, const uint32_t* off, const void* chars, uint32_t num_terms, uint32_t* out_count, uint32_t out_cap,
                       DictMatch* out);

// ---- leaf top-n of the batched suggest (dict_topn.hip): the scans' matches grouped by probe on the device, then the reference's top-n loop per probe
struct TopnProbeD {  // one top-n probe of k_dict_topn
    uint32_t rank;          // its segment of the sorted keys: seg[2 * rank], seg[2 * rank + 1]
    uint32_t top_n;         // top + skip (1 .. kTopnMax): the buffer holds at most top_n + 200 entries
    uint32_t lev;           // the clamped distance of the scoring automaton (search_field.rs:285-287)
    uint32_t check_prefix;  // 1: a hit that starts with the term gets the prefix score (:302)
    uint32_t pad[4];
};
constexpr uint32_t kTopnSlack = 200;                   // sort.rs:26
constexpr uint32_t kTopnMax = 2048 - kTopnSlack;       // the kernel's LDS buffer: 2048 entries of 8 bytes
constexpr uint32_t kTopnClasses = 512;                 // 2 * distance (u8) + prefix_matches
size_t dict_topn_sort_tmp_bytes(uint32_t n, uint32_t n_ranks);  // temporary storage of the grouping sort, size_t(-1) on an error
// recs[0, n) -> keys rank_of[probe] << 32 | term with `info` as value, sorted ascending into keys_sorted / infos_sorted; seg (2 * n_ranks + 1 words):
// every rank's [begin, end) in the sorted arrays, then the records of the ranks below n_full.  false: the sort could not be queued
bool launch_dict_topn_group(hipStream_t st, const DictMatch* recs, uint32_t n, const uint32_t* rank_of, uint32_t n_ranks, uint32_t n_full, unsigned long long* keys_in,
                            unsigned long long* keys_sorted, uint32_t* infos_in, uint32_t* infos_sorted, void* tmp, size_t tmp_bytes, uint32_t* seg);
// one wave per probe; class_ord[kTopnClasses]: 0xFFFF - rank of the class's score among the distinct scores.  The buffers are packed: probe p gets
// min(its matches, top_n + 200) entries of `out` from out_off[p] on (out_off: n_probes + 1 words, the last the total, never more than the
// records there are) and writes out_n[p] entries (class << 32 | term) there
void launch_dict_topn(hipStream_t st, const TopnProbeD* probes, uint32_t n_probes, uint32_t max_top_n, const unsigned long long* keys, const uint32_t* infos,
                      const uint32_t* seg, const uint16_t* class_ord, uint32_t* out_off, uint32_t* out_n, unsigned long long* out);
int debug_dict_topn(const uint32_t* terms, const uint32_t* classes, uint32_t n, uint32_t top_n, const uint16_t* class_ord_host, uint32_t* out_terms, uint32_t* out_classes,
                    uint32_t* out_n);

// ---- text ranking of the batched highlight (text_rank.hip): best matched-token score per text, then the page's texts selected per slot
struct TextRowD {  // one piece of a matched token's tokens_to_text_id row
    uint64_t start;  // first value of the piece inside the staged values
    uint32_t len;    // values of the piece (at most kTextRankSplit)
    uint32_t slot;   // the part's `best` array
    uint32_t bits;   // the token's f32 score bits: finite and > 0
    uint32_t pad;
};
constexpr uint32_t kTextRankSplit = 4096;              // values one wave streams: a longer row goes in several descriptors
constexpr uint32_t kTextRankMaxTop = 1024;             // top + skip a slot may ask for
constexpr size_t kTextRankBudget = size_t(128) << 20;  // bytes of `best` arrays (num_texts x 4 B per slot) one round may use
// best[slot * num_texts + text] = max(best, bits) for every value `text` < num_texts of every row piece (`best` zero-filled before)
void launch_text_best(hipStream_t st, const TextRowD* rows, uint32_t n_rows, const uint32_t* vals, uint32_t num_texts, uint32_t* best);
// per slot: the top_ns[slot] (<= out_stride) best non-zero entries by (bits descending, text ascending) as (text, bits) pairs at
// out_pairs[slot * out_stride * 2 ...) in no order; out_counts[2 * slot] = pairs written, out_counts[2 * slot + 1] = non-zero entries
void launch_text_select(hipStream_t st, const uint32_t* best, uint32_t num_texts, uint32_t n_slots, const uint32_t* top_ns, uint32_t out_stride, uint32_t* out_counts,
                        uint32_t* out_pairs);

// ---- doc sets (docset.hip): a caller's id set -> the image of an id-only list.  meta[0] = ids >= num_anchors, meta[1] = unique ids of the whole set
// bit `id` of the zeroed scratch bitmap is set for every id < num_anchors (ids: device memory, 4-byte aligned)
void launch_docset_mark(hipStream_t st, const uint32_t* ids, uint64_t n, uint32_t num_anchors, uint32_t* scratch, unsigned long long* meta);
// local[j] = scratch word base_word + j with the bits outside [doc_lo, doc_hi) cleared (j < words; bit 0 of local[0] is doc bitmap_base; words and
// base_word are multiples of 64), block_counts[b] = set bits of local words [16 b, 16 b + 16), meta[1] += set bits of the whole scratch bitmap
void launch_docset_count(hipStream_t st, const uint32_t* scratch, uint64_t scratch_words, uint64_t base_word, uint64_t words, uint32_t bitmap_base, uint32_t doc_lo,
                         uint32_t doc_hi, uint32_t* local, uint32_t* block_counts, unsigned long long* meta);
// rank_dir[0 .. blocks) (block counts, blocks a multiple of 64) -> their exclusive prefix sums in place, rank_dir[blocks] = the total; partials: blocks / 64 words
void launch_docset_scan(hipStream_t st, uint32_t* rank_dir, uint64_t blocks, uint32_t* partials);
// tile_dir[k] = rank_dir[min(k << (kTileDirShift - kRankShift), blocks)] for k < entries
void launch_docset_tiles(hipStream_t st, const uint32_t* rank_dir, uint64_t blocks, uint32_t* tile_dir, uint64_t entries);
// docs[rank] = every set bit of the local bitmap as a doc id, ascending, then 0xFFFFFFFF up to a multiple of 4 entries
void launch_docset_expand(hipStream_t st, const uint32_t* local, const uint32_t* rank_dir, uint64_t words, uint32_t bitmap_base, uint32_t* docs);
// ---- doc sets from a filter (docset_filter.hip): bit `doc` of the zeroed scratch bitmap is set for every doc the presence-only postfix program
// fops[0 .. n_fops) over lists[0 .. n_lists) selects (both in device memory; OP_LEAF = the union of its lists, OP_AND / OP_OR over nchild stack
// entries).  The program never holds more than stack_depth <= kStackDepth entries and leaves one; every list index lies below n_lists; the lists
// hold docs of [doc_lo, doc_hi) only, their bitmaps and directories start at doc_lo rounded down to 65536.  scratch_words: a multiple of 16
void launch_docset_filter(hipStream_t st, const DList* lists, uint32_t n_lists, const DOp* fops, uint32_t n_fops, uint32_t stack_depth, uint32_t doc_lo, uint32_t doc_hi,
                          uint32_t* scratch, uint64_t scratch_words);
// ---- doc set algebra (docset_algebra.hip): the scratch bitmap filled from staged sets.  An operand: its bitmap image (null: the set carries none;
// `words` words from the index's bitmap base on) and its sorted local ids (16-byte aligned, padded to a multiple of 4 entries, all inside
// [doc_lo, doc_hi)).  A launch takes up to kSetOpTable operands; the caller runs longer lists in rounds
struct SetOperand {
    const uint32_t* bitmap;
    const uint32_t* docs;
    uint32_t len, pad;
};
constexpr uint32_t kSetOpTable = 8;
struct SetOpTable {
    SetOperand o[kSetOpTable];
};
// local word j (scratch word base_word + j, as far as the scratch bitmap reaches) = is_or ? old | o[0] | .. | o[n - 1]
//   : (init_ones ? ~0 : old) & o[0] & .. & o[n_pos - 1] & ~(o[n_pos] | .. | o[n - 1]) & the bits inside [doc_lo, doc_hi).  Every operand has a bitmap
void launch_setop_words(hipStream_t st, const SetOperand* ops, uint32_t n_pos, uint32_t n, bool is_or, bool init_ones, uint32_t* scratch, uint64_t scratch_words, uint64_t base_word,
                        uint64_t words, uint32_t bitmap_base, uint32_t doc_lo, uint32_t doc_hi);
// bit `id` of the scratch bitmap cleared for each of the n ids (an operand's docs)
void launch_setop_clear(hipStream_t st, const uint32_t* ids, uint32_t n, uint32_t* scratch);
// every id of `leader` (an operand's docs) against ops[0 .. n): it survives when all hold it (negate: when none does).  refine false: survivors
// are or-ed into the zeroed scratch bitmap; true: the ids that do not survive are cleared from it
void launch_setop_probe(hipStream_t st, const uint32_t* leader, uint32_t leader_len, const SetOperand* ops, uint32_t n, bool negate, bool refine, uint32_t bitmap_base,
                        uint32_t* scratch);
// ---- facet counts of a doc set (docset_facets.hip): the histograms of m facets over a staged set's local ids, with the counting semantics of the
// scans' facet stage.  A facet's source is an anchor-keyed CSR (offsets u64 [num_keys + 1], values u32) or, for a scalar field, a direct array
// (u32 [num_keys], 0xFFFFFFFF = no value); its counters are hist[hist_off, + num_values)
struct DocsetFacetD {
    const uint64_t* offsets;
    const uint32_t* values;
    const uint32_t* direct;  // non-null: read instead of offsets / values
    uint32_t key_base, num_keys;
    uint32_t num_values;
    uint32_t hist_off;
    uint32_t lds;  // 1: the LDS mode (num_values <= kDocsetFacetLdsValues), 0: the cache mode
    uint32_t pad;
};
// Counters of a histogram that lives in LDS whole: 16 KB per workgroup of one wave, so 10 workgroups share a CU's 160 KB (2.5 waves per SIMD)
constexpr uint32_t kDocsetFacetLdsValues = 4096;
// docs: a set's sorted local ids (16-byte aligned, padded to a multiple of 4 entries), local_len of them; facets: m descriptors in device memory;
// hist: zeroed.  One launch for all m facets; nothing is launched for an empty set or an empty facet list
void launch_docset_facet_count(hipStream_t st, const uint32_t* docs, uint32_t local_len, const DocsetFacetD* facets, uint32_t m, uint32_t* hist);
// the top entries of the counted histograms: launch_facet_select's kernels and arguments
void launch_docset_facet_rank(hipStream_t st, uint32_t n_jobs, const FacetJob* jobs, const uint32_t* hist, uint32_t* out_vals, uint32_t* out_counts, uint32_t* out_n);
// ---- doc sets from numeric ranges (docset_ranges.hip): the scratch bitmap filled from column values.  A clause: a dense f32 column (bit patterns)
// with an optional presence bitmap, keyed by doc (row = doc - key_base; no value: doc < key_base, row >= num_keys, presence bit clear), and a closed
// interval [lo, hi] of range_key values, lo > hi: empty; a doc without a value holds when `missing` is set.  bitmap != 0: a 1:n clause resolved by
// launch_range_scatter — `values` is its in-range bitmap and `present` its has-a-value bitmap (null: not wanted), both of the scratch bitmap's
// shape (word doc >> 5); the clause holds for a doc in `values` or not in `present`.  A launch takes up to kRangeClauseTable clauses, a doc must
// satisfy all of them; the caller runs longer lists in passes
struct RangeClauseD {
    const uint32_t* values;
    const uint32_t* present;
    uint32_t key_base, num_keys;
    uint32_t lo, hi;
    uint32_t missing, bitmap;
};
constexpr uint32_t kRangeClauseTable = 8;
struct RangeClauseTable {
    RangeClauseD c[kRangeClauseTable];
};
// The order-preserving key of an f32 bit pattern: the sign-flipped pattern with -0 folded onto +0.  key(-inf) = 0x007FFFFF <= the key of every
// number <= key(+inf) = 0xFF800000; every NaN lies outside.  (constexpr: the host and the kernels share it)
constexpr uint32_t range_key(uint32_t bits) { return bits == 0x80000000u ? 0x80000000u : (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
constexpr uint32_t kRangeKeyMin = 0x007FFFFFu, kRangeKeyMax = 0xFF800000u;
// scratch words (doc >> 5) of the 64-doc groups that touch [doc_lo, doc_hi) = ballots of "all n clauses hold and mask holds the doc", the bits
// outside the range zero.  mask: null (all docs), or words with doc's bit in word (doc >> 5) - mask_word0; it may be `scratch` itself (and-into).
// A group whose docs are all masked is not written: its words must be zero already.  doc_hi <= the anchors the scratch bitmap covers
void launch_range_bits(hipStream_t st, const RangeClauseD* clauses, uint32_t n, const uint32_t* mask, uint32_t mask_word0, uint32_t* scratch, uint64_t scratch_words,
                       uint32_t doc_lo, uint32_t doc_hi);
// every id of `ids` (a set's docs: sorted, 16-byte aligned, padded to a multiple of 4 entries) against the n column clauses.  refine false: the ids
// that satisfy all are or-ed into the zeroed scratch bitmap; true: the ids that do not are cleared from it
void launch_range_probe(hipStream_t st, const uint32_t* ids, uint32_t len, const RangeClauseD* clauses, uint32_t n, bool refine, uint32_t* scratch);
// a 1:n clause: `column` is keyed by value id, a value belongs to the anchor in the first entry of its row of the value_id_to_anchor table (a_off
// u64 [a_num_keys + 1], a_vals; row r = value id a_key_base + r; empty rows belong to nobody).  in_bits: bit `anchor` set for every present value
// inside the interval; has_bits (null: not wanted): for every present value.  Both zeroed, of the scratch bitmap's shape; anchors outside
// [doc_lo, doc_hi) set nothing
void launch_range_scatter(hipStream_t st, const RangeClauseD& column, const uint64_t* a_off, const uint32_t* a_vals, uint32_t a_key_base, uint32_t a_num_keys, uint32_t doc_lo,
                          uint32_t doc_hi, uint32_t* in_bits, uint32_t* has_bits);
// ---- numeric aggregations of a doc set (docset_aggs.hip): counters, min / max keys, an exact sum and range-bucket counts of f32 columns over a
// staged set.  An aggregation's state is kAggBuckets + n_edges + 1 u64 slots from state[state_off] on (zeroed before the launch):
//   kAggCount    present non-NaN values (the infinities included)      kAggHas   1:n only: docs of the set with a present value
//   kAggNan      present NaNs                                          kAggMissing   anchor-keyed only: docs of the set without a value
//   kAggPosInf / kAggNegInf   the infinities among kAggCount
//   kAggLimbs    the exact sum of the finite values: 9 limbs of the positive values, then 9 of the negative ones.  A finite non-zero f32 is
//                m * 2^(s - 149), m < 2^24, s = max(biased exponent, 1) - 1 in [0, 253]; w = (u64)m << (s & 31) adds w & 0xFFFFFFFF to limb s >> 5
//                and w >> 32 to the next: the limbs weigh 2^(32 i - 149).  An addend is below 2^32 and a set holds fewer than 2^32 values: no slot
//                overflows, every sum is an integer, the result does not depend on the order of the atomics
//   kAggBuckets  bucket b = the values with exactly b edge keys <= range_key(value): edges (device memory, n_edges <= kAggMaxEdges) ascend
// and mm[mm_off] / mm[mm_off + 1] are the smallest / largest range_key counted (0xFFFFFFFF / 0 before the launch).
constexpr uint32_t kAggMaxEdges = 1023;
constexpr uint32_t kAggCount = 0, kAggMissing = 1, kAggHas = 1, kAggNan = 2, kAggPosInf = 3, kAggNegInf = 4, kAggLimbs = 5, kAggLimbsPerSign = 9;
constexpr uint32_t kAggBuckets = kAggLimbs + 2 * kAggLimbsPerSign;
struct DocsetAggD {
    const uint32_t* values;   // the column's f32 bit patterns (1:n: 16-byte aligned, a vector of slack behind them)
    const uint32_t* present;  // presence bitmap over the rows, or null: every row is present
    const uint32_t* edges;    // n_edges ascending range_key values
    const uint64_t* a_off;    // 1:n: the value_id_to_anchor table (row r = value id a_key_base + r), the first entry of a row is the value's anchor
    const uint32_t* a_vals;
    uint32_t* has_bits;       // 1:n: a zeroed bitmap of the scratch bitmap's shape (word doc >> 5)
    uint32_t key_base, num_keys;
    uint32_t a_key_base, a_num_keys;
    uint32_t n_edges, state_off, mm_off, pad;
};
// anchor-keyed columns (row = id - key_base; no value: id < key_base, row >= num_keys, presence bit clear): workgroup (x, f) aggregates aggs[f]
// over its stride of the set's local ids (docs: sorted, 16-byte aligned, padded to a multiple of 4 entries).  prereduce: the sum's addends of a
// wave's round are added up per limb across the wave before they reach LDS; false: one LDS atomic pair per value.  Nothing is launched for an
// empty set or list.  max_grid: workgroups per aggregation at most (0: kAggMaxGrid, docset_aggs.hip)
void launch_docset_agg_ids(hipStream_t st, const uint32_t* docs, uint32_t local_len, const DocsetAggD* aggs, uint32_t m, unsigned long long* state, uint32_t* mm, bool prereduce,
                           uint32_t max_grid = 0);
// 1:n columns (keyed by value id): workgroup (x, f) streams its stride of aggs[f]'s column; a present value whose anchor lies in [doc_lo, doc_hi)
// and in `member` (bit of doc d in word (d >> 5) - member_word0) is aggregated, and sets its anchor's bit in has_bits: the first to set it counts
// the doc in kAggHas.  max_keys: the largest num_keys of the m columns
void launch_docset_agg_values(hipStream_t st, const DocsetAggD* aggs, uint32_t m, uint32_t max_keys, const uint32_t* member, uint32_t member_word0, uint32_t doc_lo,
                              uint32_t doc_hi, unsigned long long* state, uint32_t* mm, bool prereduce, uint32_t max_grid = 0);
// ---- doc sets ordered by a column (docset_top.hip): the first K rows of a staged set's docs in the order (sort key ascending, doc ascending).
// The sort key of a doc: range_key(bits) of its value (descending: ~range_key(bits); both in [kRangeKeyMin, kRangeKeyMax]), kTopNanKey for a NaN,
// kTopMissingKey for a doc without a value; a 1:n doc gets the smallest sort key of its present values.  A call owns its scratch:
//   keys    the sort key of every local id (u32, local_len rounded up to whole 16-byte vectors; the padding holds kTopMissingKey, never counted)
//   hist    4 histograms of 256 bins, one per byte of the key from the top byte down (zeroed before the launch)
//   chunks  per workgroup of the tie kernels the keys == T of its contiguous chunk
//   state   kTopStateWords u32 (zeroed, or preset for a call without select): the three counters, the emit cursor, the agreed prefix, the rows
//           still wanted, then the outcome of the select: the threshold key T, B = keys < T, E = keys == T, the ties to take (rows wanted - B),
//           whether all ties are taken (E == take: they go through the cursor), done (nothing is wanted: nothing is emitted)
constexpr uint32_t kTopNanKey = 0xFFFFFFFEu, kTopMissingKey = 0xFFFFFFFFu;
constexpr uint32_t kTopMaxRows = 65536;  // top + skip of one call: the search's own bound on ranked hits
constexpr uint32_t kTopMaxGrid = 2048;   // workgroups of one wave per kernel; the rest of the work is strided
constexpr uint32_t kTopCount = 0, kTopNan = 1, kTopMissing = 2, kTopCursor = 3, kTopPrefix = 4, kTopWant = 5, kTopT = 6, kTopB = 7, kTopE = 8, kTopTake = 9, kTopAllTies = 10,
                   kTopDone = 11, kTopStateWords = 16;
struct DocsetTopD {
    const uint32_t* values;   // the column's f32 bit patterns (1:n: 16-byte aligned, a vector of slack behind them)
    const uint32_t* present;  // presence bitmap over the rows, or null: every row is present
    const uint64_t* a_off;    // 1:n: the value_id_to_anchor table (row r = value id a_key_base + r), the first entry of a row is the value's anchor
    const uint32_t* a_vals;
    const uint32_t* best;     // 1:n, k_top_keys: the folded sort key of doc d at best[d - doc_lo], read in place of the column
    uint32_t key_base, num_keys;
    uint32_t a_key_base, a_num_keys;
    uint32_t doc_lo, descending;
};
inline uint32_t top_grid(uint64_t vectors, uint32_t max_grid) {  // workgroups of 64 lanes, one 16-byte vector per lane and round
    const uint64_t waves = (vectors + 63u) / 64u;
    const uint32_t cap = max_grid ? (max_grid < kTopMaxGrid ? max_grid : kTopMaxGrid) : kTopMaxGrid;
    return uint32_t(waves < cap ? (waves ? waves : 1u) : cap);
}
// 1:n: best[anchor - doc_lo] = min(best, sort key) for every present value whose anchor lies in [doc_lo, doc_hi) and in `member` (bit of doc d in
// word (d >> 5) - member_word0); best: doc_hi - doc_lo words preset to kTopMissingKey
void launch_top_fold(hipStream_t st, const DocsetTopD& a, const uint32_t* member, uint32_t member_word0, uint32_t doc_hi, uint32_t* best, uint32_t max_grid);
// keys[i] = the sort key of docs[i] (docs: sorted, 16-byte aligned, padded to a multiple of 4 entries, all inside the index's doc range); hist[top
// byte] and the three counters of `state` count the local_len real entries
void launch_top_keys(hipStream_t st, const uint32_t* docs, uint32_t local_len, const DocsetTopD& a, uint32_t* keys, uint32_t* hist, uint32_t* state, uint32_t max_grid);
// one wave: the digit at `shift` (24, 16, 8, 0) of the threshold from this pass's histogram.  shift 24 first sets the rows wanted to min(rows,
// with_missing ? n : state[kTopCount]); shift 0 leaves T, B, E, take and all-ties
void launch_top_pick(hipStream_t st, uint32_t* state, const uint32_t* hist, uint32_t shift, uint32_t rows, bool with_missing, uint32_t n);
// hist[byte at shift] += 1 for every of the n keys whose higher bytes equal state[kTopPrefix] (shift 16, 8, 0)
void launch_top_hist(hipStream_t st, const uint32_t* keys, uint32_t n, uint32_t shift, const uint32_t* state, uint32_t* hist, uint32_t max_grid);
// the ties: workgroup c owns the vectors [c * vpc, (c + 1) * vpc) of keys / docs, vpc = ceil(vectors / grid), grid = top_grid(vectors, max_grid) in
// both launches.  chunks[c] = its keys == T (left alone when all ties are taken or none is)
void launch_top_tiecount(hipStream_t st, const uint32_t* keys, uint32_t n, const uint32_t* state, uint32_t* chunks, uint32_t max_grid);
// out[..] = key << 32 | doc: every key < T through the cursor (no order), then the first `take` keys == T in doc order at out[B ..); when all ties
// are taken they go through the cursor too.  Nothing is written at or behind out[cap]
void launch_top_emit(hipStream_t st, const uint32_t* docs, const uint32_t* keys, uint32_t n, uint32_t* state, const uint32_t* chunks, unsigned long long* out, uint32_t cap,
                     uint32_t max_grid);

// ---- text locality pre-pass (K7)
struct LocRow {  // copy table[src .. src + len) to the gather buffer at dst
    uint64_t src, dst;
    uint32_t len, pad;
};
struct LocJob {  // one (request, field): its slice [seg_begin, seg_end) of the gathered text ids, its text_id_to_anchor rows, its output ranges
    const uint32_t* t2a_vals;
    const uint64_t* t2a_start;
    const uint32_t* t2a_len;
    uint32_t t2a_key_base, t2a_num_keys;
    uint32_t seg_begin, seg_end;
    uint32_t pair_begin, pair_end;  // slice of the (anchor, boost) pair buffer (known after the count pass)
    uint32_t out_off, pad;          // first entry of the job's result inside the output arrays
};
void launch_loc_gather(hipStream_t st, const LocRow* rows, uint32_t n_rows, const uint32_t* table, uint32_t* gathered);
void launch_loc_expand(hipStream_t st, bool write, const LocJob* jobs, uint32_t n_jobs, const uint32_t* sorted_text_ids, uint32_t n, uint32_t* totals_or_cursors,
                       unsigned long long* pairs);
void launch_loc_compact(hipStream_t st, const LocJob* jobs, uint32_t n_jobs, const unsigned long long* sorted_pairs, uint32_t* out_docs, float* out_vals, uint32_t* out_len);
size_t seg_sort_u32(void* tmp, size_t tmp_bytes, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t nseg, const uint32_t* seg_begin, const uint32_t* seg_end,
                    hipStream_t st);
size_t seg_sort_u64(void* tmp, size_t tmp_bytes, const unsigned long long* in, unsigned long long* out, uint32_t n, uint32_t nseg, const uint32_t* seg_begin,
                    const uint32_t* seg_end, hipStream_t st);

// ---- 1:n boost lists (K10, boost.rs:432-468)
struct B1nJob {  // sorted value ids [seg_begin, seg_end) -> the (anchor, boost value) pair of every boosted one, in value-id order
    const uint32_t* boost_present;  // bitmap over [boost_key_base, + boost_num_keys), or null = all present
    const float* boost_values;
    const uint64_t* to_anchor_off;  // value_id_to_anchor as a CSR
    const uint32_t* to_anchor_vals;
    uint32_t boost_key_base, boost_num_keys, to_anchor_key_base, to_anchor_num_keys;
    uint32_t seg_begin, seg_end, out_off, doc_lo, doc_hi, pad;
};
struct B1nResult {
    uint32_t len, total, flags, pad;  // pairs inside [doc_lo, doc_hi) / in all; flags: 1 anchors not ascending, 2 an anchor with several values
};
void launch_b1n_map(hipStream_t st, const B1nJob* jobs, uint32_t n_jobs, const uint32_t* sorted_value_ids, uint32_t* out_docs, float* out_vals, B1nResult* results);

// ---- explain: the returned hits' scores recomputed step by step, every intermediate value written to a trace
struct ExList {  // one posting list of one matched term (search_field.rs:419-444)
    const uint32_t* docs;
    const uint16_t* scores;
    uint32_t len;
    float term_score;
};
constexpr uint32_t XP_LEAF = 0, XP_AND = 1, XP_OR = 2;
struct ExOp {  // postfix program of the request's score tree (not limited by the scan kernels' descriptor sizes)
    uint32_t kind, nchild;
    uint32_t a;  // LEAF: first list | AND: offset of the summation order in aux[] | OR: offset of the operands' term slots in aux[]
    uint32_t b;  // LEAF: lists | OR: term slots
};
struct ExQuery {
    uint32_t op_begin, n_ops, list_begin, n_lists, col_begin, n_col;
    uint32_t doc_begin, trace_begin;  // first doc of the query in docs[]; first trace word of that doc
};
constexpr uint32_t kExStack = 256;  // operands alive at once
// trace of one doc, 3 words per entry: lists {f16 bits or 0xFFFFFFFF, anchor score, final score}, ops {present, value, OR: sum over the term slots},
// column boosts {applied, log10 factor, score after}, then {root present, tree score, final score}
__host__ __device__ inline uint32_t explain_trace_words(uint32_t n_lists, uint32_t n_ops, uint32_t n_col) { return 3u * (n_lists + n_ops + n_col + 1u); }
void launch_explain(hipStream_t st, uint32_t n_docs, const ExQuery* queries, const uint32_t* doc_query, const uint32_t* docs, const ExOp* ops, const uint16_t* aux,
                    const ExList* lists, const DColBoost* cols, uint32_t* trace);

#ifdef VQ_STAMP
void debug_read_stamps(unsigned long long* out, int reset);
void debug_read_probe_stamps(unsigned long long* out, int reset);
#endif

}  // namespace vq
