// Host side of the MI355X query path: staged index image, query compiler, batch executor.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <limits>
#include <memory>
#include <thread>
#include <functional>
#include <condition_variable>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "device_types.hpp"
#include "kernels.hpp"
#include "request.hpp"
#include "hostpool.hpp"
#include "regex_dfa.hpp"

struct vq_shard_step;  // shard_step.cpp

namespace vq {

using vqreq::VelociError;

#define VQ_HIP(expr)                                                                                                          \
    do {                                                                                                                      \
        hipError_t _e = (expr);                                                                                               \
        if (_e != hipSuccess) throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr); \
    } while (0)

// small helpers the executor's translation units share (exec.cpp, prepass.cpp)
inline bool timing_enabled() {
    static const bool on = std::getenv("VQ_TIMING") != nullptr;
    return on;
}
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// suffix constants, reference src/persistence.rs:23-50
extern const char* const TOKENS_TO_TEXT_ID;
extern const char* const TO_ANCHOR_ID_SCORE;
extern const char* const PHRASE_PAIR_TO_ANCHOR;
extern const char* const VALUE_ID_TO_PARENT;
extern const char* const PARENT_TO_VALUE_ID;
extern const char* const TEXT_ID_TO_ANCHOR;
extern const char* const ANCHOR_TO_TEXT_ID;
extern const char* const BOOST_VALID_TO_VALUE;
extern const char* const VALUE_ID_TO_ANCHOR;
extern const char* const TEXTINDEX;
extern const char* const TOKEN_VALUES;

// ------------------------------------------------------------------ builder-side (host copies of what the caller hands over)
struct HostFst {
    std::vector<std::string> terms;  // bytewise sorted, ordinal == term id
};
// blocks of 64 MiB and more straight from mmap, as transparent huge pages where the kernel offers them: staging faults in and gives back tens
// of gigabytes, 512 times fewer pages to map and unmap
void* big_alloc(size_t bytes);
void big_free(void* p, size_t bytes) noexcept;
constexpr size_t kBigAlloc = size_t(64) << 20;

// resize() leaves the elements uninitialised: staging overwrites every element of its big arrays (on several threads), a zero fill first would be
// a single-threaded pass over tens of gigabytes
template <class T>
struct UninitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = UninitAlloc<U>;
    };
    UninitAlloc() = default;
    template <class U>
    UninitAlloc(const UninitAlloc<U>&) noexcept {}
    T* allocate(size_t n) {
        return n * sizeof(T) >= kBigAlloc ? static_cast<T*>(big_alloc(n * sizeof(T))) : std::allocator<T>::allocate(n);
    }
    void deallocate(T* p, size_t n) noexcept {
        if (n * sizeof(T) >= kBigAlloc) big_free(p, n * sizeof(T));
        else std::allocator<T>::deallocate(p, n);
    }
    template <class U>
    void construct(U* p) noexcept {
        ::new (static_cast<void*>(p)) U;
    }
    template <class U, class... A>
    void construct(U* p, A&&... a) {
        ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
    }
};
template <class T>
using uninit_vector = std::vector<T, UninitAlloc<T>>;

// host threads per index for request compilation and staging (the caller counts as one): VQ_HOST_THREADS, else the machine's, at most 16
size_t host_threads();
// fn(i) for i in [0, n) on `threads` threads (the caller included), items claimed one at a time; the first exception is rethrown
void parallel_for(size_t n, size_t threads, const std::function<void(size_t)>& fn);

struct HostPostings {
    std::vector<uint64_t> offsets;
    uninit_vector<uint32_t> anchors;
    uninit_vector<uint32_t> scores;
    std::vector<uint64_t> global_lens;  // empty: lengths of the arrays handed over are the global ones
};
struct HostKV {
    uint32_t key_base = 0;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> values;
};
struct HostPhrase {
    std::vector<uint32_t> t1, t2;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> anchors;
};
struct HostBoost {
    uint32_t key_base = 0;
    std::vector<uint8_t> present;
    std::vector<uint32_t> bits;
};
struct ColumnMeta {
    bool is_anchor_identity_column = false;
    bool tokenize = true;
};

struct IndexBuilder {
    uint32_t num_anchors = 0, doc_lo = 0, doc_hi = 0;
    std::map<std::string, HostFst> fst;
    std::map<std::string, HostPostings> postings;
    std::map<std::string, HostKV> kv;
    std::map<std::string, HostPhrase> phrase;
    std::map<std::string, HostBoost> boost;
    std::map<std::string, ColumnMeta> columns;
};

// ------------------------------------------------------------------ staged image
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            bytes = o.bytes;
            o.p = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void alloc(size_t n);
    void ensure(size_t n);  // grow (never shrink); contents are not preserved
    void release();
    void upload(const void* src, size_t n, hipStream_t st = nullptr);
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

struct Dictionary {  // term dictionary of one text field
    std::vector<std::string> terms;
    std::unordered_map<std::string, std::vector<uint32_t>> lower_map;  // lowercase(term) -> ascending term ids (exact lookups)
    // device image for the fuzzy / prefix scan (k_dict_scan): one code point per element, raw and lower-cased per code point
    uint32_t char_bytes = 2;  // 2: every code point is below U+10000 (u16 image); 4: some term has one above U+FFFF (u32 image)
    size_t max_term_bytes = 0;  // the longest term (the batched suggest's top-n route wants every term shorter than 200 bytes)
    bool low_exact = true;    // false: the lower-cased image is not str::to_lowercase of every term (U+0130): matches are scored on the host
    DevBuf d_off;             // u32 [T + 1]
    DevBuf d_raw;             // u16 or u32 (char_bytes)
    DevBuf d_low;             // u16 or u32 (char_bytes)
    // regex leaves (k_dict_regex): the distinct code points of the terms, ascending; the device holds the part from U+0080 on
    std::vector<uint32_t> alphabet;
    uint32_t alphabet_ascii = 0;  // entries of `alphabet` below 128
    DevBuf d_alpha;               // u32 [alphabet.size() - alphabet_ascii]
    std::unique_ptr<vqregex::AtomCache> regex_atoms;  // (atom text, icase) -> members of the alphabet, filled by the leaves that ask
};

struct Index;
struct PostingStore;
struct FuzzyProbe {  // one dictionary scan of a batch (get_text_lines_from_fst, search_field.rs:68-99)
    std::string key;
    std::string path;                 // "<field>.textindex"
    std::vector<uint32_t> query;      // code points of the ORIGINAL term (lower-cased when case-insensitive)
    uint32_t max_d = 0;
    bool transposition = false, prefix = false, ci = true;
    std::vector<uint32_t> matches;    // ascending term ids == FST stream order
    std::vector<float> scores;        // default_score_for_distance of every match (search_field.rs:304-321), scored once per batch
    std::string lower_term;           // scoring side: the lower-cased term, the clamped distance, the prefix rule (:284-302)
    uint32_t lev = 0;
    bool check_prefix = false;
    int status = 0;
    std::string error;
    bool regex = false;               // a regex leaf whose pattern compiled (k_dict_regex): `dfa` is the probe, `matches` the result, scores stay with the host
    vqregex::Dfa dfa;
    bool answered = false;            // run_fuzzy_probes has filled `matches`
    // > 0: a top-n probe of the batched suggest (top + skip of its part).  `matches` / `scores` are then NOT a match set: they are the final buffer
    // of the reference's top-n loop (search_field.rs:322-333) in buffer order, at most top_n + 200 entries, made by k_dict_topn.  Its key carries
    // top_n (topn_key), so nothing that looks a probe up by fuzzy_key finds it.
    uint32_t top_n = 0;
    uint32_t topn_copied = 0;  // entries copied back for it: min(its matches, top_n + 200)
};
using FuzzyTable = std::map<std::string, FuzzyProbe>;
std::string fuzzy_key(const vqreq::RequestSearchPart& p);
std::string topn_key(const vqreq::RequestSearchPart& p);  // fuzzy_key plus top + skip: the key of a part's top-n probe
bool needs_dictionary_scan(const vqreq::RequestSearchPart& p);
// The route of a regex part: its DFA when k_dict_regex takes it, else the reason it stays on the host.  Throws what the search would answer for
// a part that cannot run at all (no terms, unknown field, invalid pattern).
vqregex::Compiled regex_route(const Index& idx, const vqreq::RequestSearchPart& p);
void collect_fuzzy_probes(const Index& idx, const vqreq::Request& req, FuzzyTable& table);
struct Workspace;
void run_fuzzy_probes(const Index& idx, Workspace& ws, FuzzyTable& table, hipStream_t st);
void score_fuzzy_probe(const Index& idx, FuzzyProbe& probe);
float default_score_for_distance_host(uint8_t distance, bool prefix_matches);  // search_field.rs:27-33
size_t debug_sort_unique(uint32_t* ids, size_t n);
struct SuggestEntry {  // search_field.rs:158 SuggestFieldResult = Vec<(String, Score, TermId)>
    std::string text;
    float score;
    uint32_t term_id;
};
// (topn_probes: `fuzzy` is the table of a suggest batch and may hold the part's top-n probe)
std::vector<SuggestEntry> suggest_part(const Index& idx, const vqreq::RequestSearchPart& part, const FuzzyTable* fuzzy, bool topn_probes = false);
void collect_suggest_probes(const Index& idx, const vqreq::Request& req, FuzzyTable& table);
// the same for a request of a suggest batch: a part that qualifies gets a top-n probe instead of a full one
void collect_suggest_batch_probes(const Index& idx, const vqreq::Request& req, FuzzyTable& table);
void topn_class_ords(uint16_t* ord);  // k_dict_topn's class table (kTopnClasses entries), as the suggest batch uploads it
bool probe_scored_on_device(const Index& idx, const FuzzyProbe& fp);  // run_fuzzy_probes' rule: the scan kernel scores the hits of this probe
std::optional<std::string> highlight_text(const std::string& text, const std::vector<std::string>& terms, const vqreq::SnippetInfo& opt, bool tokenized);  // highlight_field.rs:92-146
vqreq::Request page_request_after(const vqreq::Request& request, float score, uint32_t id);
// highlight_part in its two steps (the batched highlight runs them apart): the part's matched tokens with their scores (get_term_ids_in_field +
// token_value), then resolve_token_hits_to_text_id with snippets over the host stores
struct HighlightLookup {
    std::string path;                                      // "<field>.textindex"
    std::vector<std::pair<uint32_t, float>> hits_scores;   // (token id, score)
    bool tokenized = false, add_snippets = false;
};
HighlightLookup highlight_lookup(const Index& idx, const vqreq::RequestSearchPart& part, const FuzzyTable* fuzzy);
std::vector<SuggestEntry> highlight_resolve(const Index& idx, const vqreq::RequestSearchPart& part, const HighlightLookup& lk);
std::vector<SuggestEntry> highlight_part(const Index& idx, const vqreq::RequestSearchPart& part, const FuzzyTable* fuzzy);
// the snippet of `text` of field `lk.path` for the matched tokens `wanted_sorted` (highlight_document, highlight_field.rs:187-272); false: none
bool highlight_snippet(const Index& idx, const HighlightLookup& lk, const vqreq::RequestSearchPart& part, uint32_t text, const std::vector<uint32_t>& wanted_sorted, std::string* out);
std::vector<SuggestEntry> run_highlight(const Index& idx, vqreq::RequestSearchPart part);  // search_field::highlight, search_field.rs:233-245
std::vector<SuggestEntry> run_suggest(const Index& idx, const vqreq::Request& req);  // suggest_multi, search_field.rs:194-219
// n highlight parts as one device batch (a null part fails alone); every result equals run_highlight's.  A part that qualifies has
// its texts ranked and cut to the page on the device (text_rank.hip) and only the page's snippets built
void run_highlight_batch(const Index& idx, const vqreq::RequestSearchPart* const* parts, size_t n, std::vector<std::vector<SuggestEntry>>& out, std::vector<int>& status,
                         std::vector<std::string>& errors);
// k_text_best + k_text_select alone on a caller's CSR (vq_debug_text_rank): rows [row_off[r], row_off[r + 1]) of `vals` with score bits[r] -> the
// top_n texts sorted by (bits descending, text ascending) and the number of touched texts.  Throws without a device
void debug_text_rank(const uint64_t* row_off, const uint32_t* vals, const uint32_t* bits, uint32_t num_rows, uint32_t num_texts, uint32_t top_n,
                     std::vector<std::pair<uint32_t, uint32_t>>& picked, uint32_t* touched);
// k_merge_spans / k_finalize alone on crafted host tables, all jobs in one launch (vq_debug_merge_spans / vq_debug_finalize, which check the
// arguments; include/veloci_amd.h describes the tables).  Throw without a device
void debug_merge_spans(const uint64_t* span_keys, const uint32_t* n_spans, const uint32_t* top_k, uint32_t n_jobs, uint64_t* out_keys);
void debug_finalize(const uint64_t* shard_keys, const uint64_t* shard_hits, uint32_t num_shards, size_t stride_pad, const uint32_t* top_k, uint32_t n_jobs,
                    uint32_t* out_ids, uint32_t* out_score_bits, uint32_t* out_n, uint64_t* out_hits);
// n suggest requests as one device batch (a null request, or one that fails, fails alone: status / errors); every result equals run_suggest's
void run_suggest_batch(const Index& idx, const vqreq::Request* const* reqs, size_t n, std::vector<std::vector<SuggestEntry>>& out, std::vector<int>& status,
                       std::vector<std::string>& errors);

// A leaf whose expansion matched many terms is materialised before the scan (k_union, K2): union of the
// terms' posting lists with the per-doc maximum of term_score * (f16 / 100).
struct UnionJob {
    std::string key;
    struct Term {
        const PostingStore* store;  // "<field>.textindex.to_anchor_id_score" of the term's field (a fused leaf spans several fields)
        uint32_t token;
        float score;                // term score
    };
    std::vector<Term> terms;                           // the lists to merge (those with entries in the unsharded index)
    // result (valid until the batch that ran it is finished; lives in the batch workspace)
    const uint32_t* d_docs = nullptr;
    const float* d_vals = nullptr;
    float max_value = std::numeric_limits<float>::infinity();  // largest value of the merged list (read back after the write pass)
    uint32_t len = 0;
    uint64_t global_len = 0;  // merged length over all shards
    uint64_t input_postings = 0;
};
using UnionTable = std::map<std::string, UnionJob>;
// Leaf hits inside doc ranges, counted before the final compilation (k_range_hits): the reference's merge of a 1:n boost list into a
// leaf's hits applies the first or all of an anchor's values depending on the hits around that anchor (boost.rs:255-281).
struct RangeJob {
    std::string key;
    std::string store_path;          // "<field>.textindex.to_anchor_id_score"
    std::vector<uint32_t> tokens;    // the leaf's posting lists
    std::string union_key;           // key of the leaf's union job when it asks to be materialised (the merged list is scanned instead)
    std::shared_ptr<const std::vector<uint32_t>> anchors;  // the boost list's entry anchors a_0 < a_1 < ... (owned by the batch's Boost1nEntry)
    std::vector<uint64_t> counts;    // result, summed over the shards: [2j] leaf postings at a_j, [2j + 1] strictly between a_(j-1) and a_j (0 for j = 0)
};
using RangeTable = std::map<std::string, RangeJob>;
// (anchor, boost value) lists of 1:n field boosts resolved on the host, shared by the requests and compilation passes of one batch
// One 1:n boost list of a batch (boost.rs:432-468 resolved for one leaf request and boost path), shared by the compilation passes and by every
// request of the batch with that leaf: the (anchor, value) pairs, what the compiler needs to know about their order, and — once known — the
// layers the device applies (one sorted unique list per applied value of an anchor).
struct Boost1nEntry {
    struct Layer {
        std::vector<uint32_t> docs;
        std::vector<float> vals;
        uint64_t global_len = 0;
    };
    std::once_flag resolved, layered;
    std::vector<std::pair<uint32_t, float>> pairs;
    bool ascending = true, several = false;
    std::vector<uint32_t> anchors;  // several: the distinct anchors, ascending
    std::shared_ptr<const std::vector<Layer>> layers;
};
struct Boost1nCache {  // sharded: every compiling thread comes here once per boosted leaf, and a thread that has to sleep on a lock loses more time
                       // than the lookup takes
    static constexpr size_t kShards = 64;
    struct Shard {
        std::mutex mu;
        std::unordered_map<std::string, std::shared_ptr<Boost1nEntry>> map;
    } shard[kShards];
    std::shared_ptr<Boost1nEntry> entry(const std::string& key) {
        Shard& sh = shard[std::hash<std::string>{}(key) % kShards];
        std::lock_guard<std::mutex> g(sh.mu);
        auto& slot = sh.map[key];
        if (!slot) slot = std::make_shared<Boost1nEntry>();
        return slot;
    }
    const std::map<std::string, struct Boost1nJob>* device = nullptr;  // lists the K10 pre-pass has resolved on the device (second compilation pass on)
};
// Text locality of a field whose text ids are not anchors (boost.rs:34-87), resolved before the final compilation by the K7 pre-pass: the
// token -> text rows of the query's terms are gathered and sorted, texts occurring c > 1 times are expanded to their anchors with the boost
// 2*c*c, the (anchor, boost) pairs are sorted and the smallest boost of every anchor is kept (the reference's reversed max_by, boost.rs:25).
struct LocalityJob {
    std::string key;
    std::string t2t_path, t2a_path;                   // "<field>.textindex.tokens_to_text_id" / ".text_id_to_anchor"
    std::vector<uint32_t> tokens;                     // token ids of all terms (multiplicity kept: the count is over list entries, boost.rs:51-56)
    // result (valid until the batch that ran it is finished; lives in the batch workspace)
    const uint32_t* d_docs = nullptr;
    const float* d_vals = nullptr;
    uint32_t len = 0;
};
using LocalityTable = std::map<std::string, LocalityJob>;
// A 1:n boost list (boost.rs:432-468) resolved by the K10 pre-pass: the leaf's text ids -> value ids of the 1:n object (gathered and sorted on
// the device) -> the (anchor, boost value) pair of every boosted value id, in value-id order, as a (doc, f32) list the scans read.
struct Boost1nJob {
    std::string key;
    std::string to_parent_path, to_anchor_path, boost_path;  // "<leaf>.textindex.value_id_to_parent", "<boost>.value_id_to_anchor", "<boost>.boost_valid_to_value"
    std::vector<uint32_t> text_ids;
    // result (lives in the batch workspace)
    const uint32_t* d_docs = nullptr;
    const float* d_vals = nullptr;
    uint32_t len = 0;          // pairs inside this shard
    uint32_t total = 0;        // pairs of the unsharded list
    bool ascending = true;     // anchors non-decreasing in value-id order (else the reference's merge is not reproducible: declined)
    bool several = false;      // some anchor has more than one boosted value: the look-ahead rule applies (host path)
    bool done = false;
};
using Boost1nTable = std::map<std::string, Boost1nJob>;
constexpr int kStatusNeedsUnion = -1;  // internal: compile again once the requested union / locality jobs have run
constexpr int kStatusNeedsCounts = -2; // internal: the compiled query IS a count pre-pass; compile again with its results
constexpr int kStatusNeedsRanges = -3; // internal: compile again once the requested range jobs have run

// Result sizes of the operands of AND nodes, measured by a count pre-pass (the reference orders the score sum of an AND by
// its operands' result lengths and labels an AND result by them, set_op.rs:388-393,439).
struct QueryCounts {
    bool has_filter = false;
    uint64_t filter_count = 0;                                       // ids in the filter result (Set below 100 001 ids, filter_result.rs:5-22)
    std::map<uint32_t, std::pair<uint64_t, uint64_t>> nodes;        // node id (preorder) -> (hits, hits inside the filter)
};

struct PostingStore {  // "<field>.textindex.to_anchor_id_score": padded segmented arrays in HBM
    uint32_t num_tokens = 0;
    std::vector<uint64_t> start;        // start[t]: first entry of list t inside docs/scores (multiple of 4)
    std::vector<uint32_t> len;          // entries of list t inside this shard
    std::vector<uint64_t> global_len;   // entries of list t in the unsharded index
    std::vector<uint16_t> max_raw;      // largest f16 score bits of list t (upper bound for OR pruning)
    std::vector<uint16_t> pivot_raw;    // array lists: raw scores <= this are the list's low score class (score_class_pivot); == max_raw: no class
    DevBuf docs;                        // u32, lists padded to a multiple of 4 with 0xFFFFFFFF
    DevBuf scores;                      // f16 bits (u16), same indexing
    uint64_t total_padded = 0;
    // dense lists (>= 1/64 of the shard's docs) also get a bitmap image + a rank directory
    std::vector<int64_t> bm_start;      // word offset of list t inside `bitmaps`, or -1
    std::vector<int64_t> rd_start;      // entry offset of list t inside `rank_dir`, or -1
    DevBuf bitmaps;                     // u32 words; bit (doc - Index::bitmap_base)
    DevBuf rank_dir;                    // u32: entries below bitmap_base + (k << kRankShift)
    // lists that hold at least 1/4096 of the shard's docs get a tile directory (k_scan_probe reads a tile's postings of
    // its cover list without searching or counting): entries below bitmap_base + (k << kTileDirShift)
    std::vector<int64_t> td_start;      // entry offset of list t inside `tile_dir`, or -1
    DevBuf tile_dir;
    // ... and a tile-packed image for k_scan_probe (round 4): the list's postings grouped by 32768-doc tile, every tile padded to a
    // multiple of 8 entries (a "granule"), as `cov32` = (doc - tile_lo) << 16 | f16 score (what a COVER streams: 4 B per posting, one
    // 16 B/lane load per 256 postings, no index arithmetic) and — when no tile holds more than 2048 entries — as `arr16` = (doc - tile_lo) << 1 | score class
    // (what an OPERAND of fewer than 1/16 of the docs is probed in: a sorted 16-bit array per tile, Roaring's array container, 2 B per
    // posting instead of a bit per doc).  Both share one directory: gdir[k] = granules below tile k.
    std::vector<int64_t> pk_start;      // granule offset of list t inside `cov32`, or -1
    std::vector<int64_t> ak_start;      // granule offset of list t inside `arr16`, or -1 (a tile with more than 2048 entries)
    std::vector<int64_t> gd_start;      // entry offset of list t inside `gdir`
    // An arr16 entry is (doc - tile_lo) << 1 | low (device_types.hpp: kArrPadRel), low = the posting's raw score is <= pivot_raw[t].
    std::vector<uint32_t> tile_most;    // most granules list t has in one tile (0 without a tile-packed image): sizes an array operand's LDS slot per launch
    DevBuf cov32, arr16, gdir;
};

struct KVStore {  // IndexIdToParent<u32>: host copy + (where useful) device images
    uint32_t key_base = 0, num_keys = 0;  // host addressing, as handed over
    std::vector<uint64_t> host_off;
    std::vector<uint32_t> host_values;
    // list use: values are anchors -> every row is a padded, sorted, unique doc-id list in HBM
    bool list_rows = false;
    bool rows_sorted_unique = true;
    bool rows_equal_postings = false;  // tokens_to_text_id of an identity column: row t holds exactly the docs of posting list t
    std::vector<uint64_t> start;  // first entry of row r inside `values` (multiple of 4)
    std::vector<uint32_t> len;    // entries of row r inside this shard
    DevBuf values;
    DevBuf d_row_start, d_row_len;  // text_id_to_anchor: `start` / `len` on the device (u64 / u32 per row) — text locality expands text ids there (K7)
    // text use: tokens_to_text_id of a field whose text ids are NOT anchors: the whole table as a CSR in HBM (values are text ids: replicated
    // on every shard like the dictionary), read by the text-locality pre-pass (K7)
    bool text_csr = false;
    DevBuf d_text_vals;  // u32, host_values as handed over (row r = [host_off[r], host_off[r + 1]))
    // 1:n boost use (K10): value_id_to_parent (text id -> value ids) and value_id_to_anchor (value id -> anchor) as whole CSRs in HBM: keys
    // are not anchors, so the tables are replicated on every shard like the dictionary; d_text_vals holds the values, d_csr_off the offsets
    bool value_csr = false;
    DevBuf d_csr_off;    // u64 [num_keys + 1]
    // facet use: keys are anchors -> CSR restricted to the shard's anchors
    bool facet_csr = false;
    uint32_t csr_key_base = 0, csr_num_keys = 0;
    uint32_t csr_max_value = 0;  // largest value id of the CSR (text ids of texts too long for the dictionary lie beyond it)
    DevBuf csr_direct;  // u32 [csr_num_keys], only when no anchor has more than one value: the value id or 0xFFFFFFFF (one gather per hit
                        // instead of two offsets + the value)
    DevBuf csr_off;     // u64 [csr_num_keys + 1]
    DevBuf csr_values;  // u32

    bool host_row(uint64_t key, const uint32_t** b, const uint32_t** e) const {  // IndexIdToParent::get_values
        if (key < key_base) return false;
        uint64_t r = key - key_base;
        if (r >= num_keys || host_off[r] == host_off[r + 1]) return false;
        *b = host_values.data() + host_off[r];
        *e = host_values.data() + host_off[r + 1];
        return true;
    }
};

struct PhraseStore {
    std::vector<std::pair<uint32_t, uint32_t>> keys;  // sorted
    std::vector<uint64_t> start;
    std::vector<uint32_t> len;
    DevBuf anchors;  // padded rows
};

struct BoostColumn {
    uint32_t key_base = 0, num_keys = 0;
    bool has_present = false;
    float vmin = 0.0f, vmax = 0.0f;  // smallest / largest present value (any_value false: none)
    bool any_value = false, has_nan = false;
    DevBuf values;   // f32
    DevBuf present;  // bitmap u32
    std::vector<uint32_t> host_bits;    // host copy, kept for 1:n boost columns (keys are value ids, resolved on the host)
    std::vector<uint8_t> host_present;
    bool host_value(uint64_t key, float* out) const {  // IndexIdToParent::get_value
        if (key < key_base || key - key_base >= host_bits.size()) return false;
        const size_t r = size_t(key - key_base);
        if (!host_present.empty() && !host_present[r]) return false;
        std::memcpy(out, &host_bits[r], 4);
        return true;
    }
};

struct PinnedBuf {  // page-locked host staging
    void* p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf();
    void ensure(size_t n);
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

constexpr int kWorkspaces = 4;  // batches in flight per index (host compile of one overlaps the scan of the others; the chunks of one sharded step: one each)

// Kernels the profiler accounts separately (vq_profile_json): the pre-passes, one entry per scan class, the merges.
enum KernelId : int {
    K_DICT_SCAN = 0, K_DICT_REGEX, K_DICT_TOPN_GROUP, K_DICT_TOPN, K_TEXT_BEST, K_TEXT_SELECT, K_UNION_COUNT, K_UNION_WRITE, K_UNION_DENSE_SCATTER, K_UNION_DENSE_COUNT, K_UNION_DENSE_WRITE, K_RANGE_HITS, K_COUNT_PREPASS, K_SCAN_LEAF_F32, K_SCAN_RICH, K_SCAN_PROBE, K_SCAN_AND, K_SCAN_SIMPLE, K_SCAN_UNION,
    K_SCAN_WIDE, K_TILE_SCAN, K_MERGE_SPANS, K_FINALIZE, K_FACET_SELECT, K_LOCALITY, K_BOOST1N, K_COUNT_
};
extern const char* const kKernelNames[K_COUNT_];

struct TimedLaunch {  // one profiled launch of a batch: events [begin, end] on the launch stream
    int kernel;
    uint32_t ev_begin, ev_end;
    uint64_t layout_bytes, algorithmic_bytes, queries;
};

struct Workspace {  // scratch of one in-flight batch
    std::mutex mu;
    std::atomic<bool> pinned{false};  // held by a batch that named this workspace (the chunks of a sharded step): callers that take any free one skip it
    std::vector<hipEvent_t> ev_pool;          // profiling: created on first use
    uint32_t ev_used = 0;
    std::vector<TimedLaunch> timed;           // launches of the batch in flight (profiling)
    hipEvent_t ev_done = nullptr;             // scan + span merge finished: the finish stream waits on it
    PinnedBuf h_up, h_down;
    DevBuf d_up;        // blobs + blob_off + span_base + facet jobs
    DevBuf d_span_keys;
    DevBuf d_partial;
    DevBuf d_down;      // results
    DevBuf d_union_docs[2], d_union_vals[2], d_union_max, d_union_meta;  // materialised leaves (k_union), level 1 / level 2
    DevBuf d_union_slab, d_union_dense_docs, d_union_dense_vals, d_union_dense_meta;  // materialised wide leaves (union_dense.hip): key slabs (reused from group to group), results
    DevBuf d_loc_a, d_loc_b, d_loc_pairs_a, d_loc_pairs_b, d_loc_meta, d_loc_tmp, d_loc_docs, d_loc_vals;  // text locality pre-pass (K7)
    DevBuf d_b1n_a, d_b1n_b, d_b1n_meta, d_b1n_tmp, d_b1n_docs, d_b1n_vals;                              // 1:n boost lists (K10)
    DevBuf d_probe_desc, d_probe_counts, d_probe_ids;                    // dictionary scans (k_dict_scan): kept, so that no hipFree synchronises the device mid-pipeline
    DevBuf d_regex_tabs;                                                 // regex probes (k_dict_regex): descriptors + table pool
    DevBuf d_topn_sort, d_topn_tmp, d_topn_meta, d_topn_out;             // leaf top-n of a suggest batch (dict_topn.hip): keys + infos (unsorted, sorted), rocPRIM's storage, tables, buffers
    DevBuf d_trank_best, d_trank_meta;                                   // text ranking of a highlight batch (text_rank.hip): the round's `best` arrays; descriptors, top_n table, counts + pairs
};

struct KernelProfile {
    double ms = 0;
    uint64_t launches = 0;
    uint64_t layout_bytes = 0;       // bytes THIS layout has to move for the launches (bitmap words of dense lists, 4 B per id of scattered lists,
                                     // 6 B per streamed posting, gathered bytes counted by the kernels, 8 B per returned key): roofline numerator
    uint64_t algorithmic_bytes = 0;  // SURVEY.md 8(d) accounting (6 B per posting of every list ...): what a posting-streaming design would move
    uint64_t gathered_bytes = 0;     // the part of layout_bytes read by per-hit gathers (2 B per f16 score, 4 B per f32 / column / facet value, ...)
    uint64_t queries = 0;
};
struct Profile {
    bool enabled = false;
    KernelProfile k[K_COUNT_];
    uint64_t batches = 0;
};
// RAII bracket of one launch (or a few back-to-back launches of one kernel) with two events of the workspace's pool
struct LaunchTimer {
    Workspace* ws = nullptr;
    hipStream_t st = nullptr;
    size_t slot = 0;
    LaunchTimer(bool on, Workspace& w, hipStream_t s, int kernel, uint64_t layout_bytes = 0, uint64_t algorithmic_bytes = 0, uint64_t queries = 0);
    ~LaunchTimer();
    LaunchTimer(const LaunchTimer&) = delete;
    LaunchTimer& operator=(const LaunchTimer&) = delete;
};

// A few persistent host threads for the per-request work of a batch (query compilation): spawning threads per chunk costs more
// than compiling a small chunk.

// The exchange step of a sharded search inside the library (vq_comm_*): RCCL — loaded at run time, one communicator per index / rank — or the
// caller's own all-gather / all-reduce (vq_comm_init_custom: rehearsals with several shards in one process).  Collectives run on their own
// stream between the scan stream and the finish stream, so that step i's exchange and merge overlap step i+1's scans (two steps in flight).
struct ShardComm {
    int nranks = 1, rank = 0;
    void* nccl = nullptr;  // ncclComm_t
    int (*allgather)(void* ctx, const void* local, void* gathered, size_t bytes_per_rank, void* stream) = nullptr;
    int (*allreduce_u32)(void* ctx, void* inout, size_t count, void* stream) = nullptr;
    void* ctx = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_scan[2] = {nullptr, nullptr}, ev_xchg[2] = {nullptr, nullptr}, ev_fin[2] = {nullptr, nullptr};
    vq_shard_step* unmerged = nullptr;  // the step in flight whose merge is not queued yet
    int live = 0;              // steps begun and not yet ended / freed (at most two: each holds workspaces of its own)
    DevBuf gathered[2];
    DevBuf red;  // scratch of the sums-over-shards hook (u64)
    bool busy[2] = {false, false};  // parity (workspace pair, gather buffer, events) held by a live step
    std::string failed;  // != "": a step of this communicator failed as a whole on this rank (or did not complete in time): the ranks' exchanges no longer line
                         // up, every further step is refused until the communicator is made again (vq_comm_init / vq_comm_init_custom)
    std::mutex mu;  // the hook may be called from compile threads of two steps
    ~ShardComm();
};

struct Index {
    int device = 0;
    // sums over all shards (vq_index_set_allreduce); null: requests that need them are declined on a sharded index
    int (*allreduce_fn)(void*, uint64_t*, size_t) = nullptr;
    void* allreduce_ctx = nullptr;
    bool sharded() const { return doc_lo != 0 || doc_hi != num_anchors; }
    bool can_sum_over_shards() const { return !sharded() || allreduce_fn != nullptr; }
    void sum_over_shards(std::vector<uint64_t>& v) const {
        if (!sharded() || v.empty()) return;
        if (!allreduce_fn || allreduce_fn(allreduce_ctx, v.data(), v.size()) != 0) throw vqreq::VelociError(vqreq::ERR_DEVICE, "all-reduce over the shards failed");
    }
    // batched highlight: per field ("<field>.textindex") whether tokens_to_text_id and text_id_to_token_ids describe one relation (checked on first
    // use), and the staged values of tokens_to_text_id (uploaded then, for a field whose table the index build did not stage)
    struct HighlightField {
        std::once_flag once;
        bool ok = false;
        uint32_t num_texts = 0;          // largest text id of the table + 1
        const KVStore* t2t = nullptr;    // tokens_to_text_id
        const KVStore* tokens = nullptr; // text_id_to_token_ids
        const uint32_t* d_vals = nullptr;
        DevBuf own_vals;
    };
    mutable std::mutex highlight_mu;
    mutable std::map<std::string, std::unique_ptr<HighlightField>> highlight_fields;
    mutable std::atomic<uint64_t> highlight_device_parts{0}, highlight_snippets_built{0};  // highlight batches: parts ranked on the device; snippets built (tests, tools)
    mutable std::atomic<uint64_t> suggest_topn_probes{0}, suggest_records_back{0};  // suggest batches: probes answered by k_dict_topn; match records copied back (tests, tools)
    mutable std::atomic<uint64_t> or_reruns{0};  // requests that ran a second time because k_scan_probe_or's short cut could not be confirmed (tests, tools)
    mutable std::unique_ptr<HostPool> pool;  // created on first use
    mutable std::mutex pool_mu;
    uint64_t uid = 0;  // unique among the indexes of the process (a doc set remembers the index it was made for)
    uint32_t num_anchors = 0, doc_lo = 0, doc_hi = 0;
    uint32_t bitmap_base = 0;   // doc id of bit 0 of the list bitmaps: doc_lo rounded down to 65536
    uint64_t bitmap_words = 0;  // words of one list bitmap
    std::map<std::string, Dictionary> dict;
    std::map<std::string, PostingStore> postings;
    std::map<std::string, KVStore> kv;
    std::map<std::string, PhraseStore> phrase;
    std::map<std::string, BoostColumn> boost;
    std::map<std::string, ColumnMeta> columns;
    uint64_t device_bytes = 0;
    // facets on 1:n fields without an anchor_to_text_id index (facet.rs:59-70): the chain of parent_to_value_id joins is composed
    // once per field, on first use, into one anchor-keyed CSR that the facet kernel reads like a direct index
    mutable std::mutex composed_mu;
    mutable std::map<std::string, std::unique_ptr<KVStore>> composed_facets;
    const KVStore& composed_facet(const std::vector<std::string>& steps) const;
    hipStream_t own_stream = nullptr, own_fin_stream = nullptr;
    hipStream_t pre_stream = nullptr;  // dictionary scans, union / range / count pre-passes: every one ends in a host synchronisation, so they need no
                                       // ordering with the scan stream — and on their own stream the pre-passes of batch c+1 overlap the scan of batch c
    hipStream_t stream = nullptr;      // scans + span merges
    hipStream_t own_stream2 = nullptr;  // the second chunk of a step that is cut in two, on an index that answers alone: its upload, scans and span
                                        // merge go here, beside the first chunk's on `stream` (step_scan_stream, shard_step.cpp)
    hipStream_t fin_stream = nullptr;  // shard merge, facet selection, result download (== stream when the caller set one)
    mutable std::mutex profile_mutex;
    mutable Profile profile;
    mutable Workspace ws[kWorkspaces];
    mutable std::atomic<uint32_t> next_ws{0};
    // Sharded step run as a pipeline of chunks with ONE collective: the chunks' partials are placed back to back in this arena (run_partial's
    // arena_offset), so a single all-gather of its used prefix exchanges them all; every chunk then merges out of the gathered copy with the
    // prefix's size as the shard stride.  Fixed size: a step that does not fit is told so and takes the per-chunk path.
    mutable DevBuf arena;
    static constexpr size_t kArenaBytes = 64ull << 20;
    mutable std::unique_ptr<ShardComm> comm;  // vq_comm_init / vq_comm_init_custom
    ~Index();
    bool is_anchor_identity(const std::string& textindex_path) const;
};

std::unique_ptr<Index> build_index(const IndexBuilder& b, int device);

// ------------------------------------------------------------------ doc sets
// A caller's id set staged in HBM in the image the scans read for an id-only list — byte for byte what build_index makes of a posting list's ids:
//   docs      the sorted unique ids inside [doc_lo, doc_hi), padded to a multiple of 4 entries with 0xFFFFFFFF
//   bitmap    (dense sets: range >= 65536 and local_len * 64 >= range) Index::bitmap_words words, bit (doc - bitmap_base)
//   rank_dir  (with the bitmap) entries below bitmap_base + (k << kRankShift), k = 0 .. bitmap_words / 16
//   tile_dir  (range >= 65536 and local_len * 4096 >= range) entries below bitmap_base + (k << kTileDirShift), k = 0 .. bitmap_words / 512 + 3
// Built on the device (docset.hip) by make_docset, immutable afterwards: any number of requests and threads share one.
struct DocSet {
    uint64_t index_uid = 0;  // Index::uid of the index it was made for
    uint32_t num_anchors = 0, doc_lo = 0, doc_hi = 0;
    uint64_t len = 0;        // unique ids of the whole set (the same on every shard)
    uint32_t local_len = 0;  // those inside [doc_lo, doc_hi)
    uint64_t bitmap_words = 0, rank_entries = 0, tile_entries = 0;  // elements of the parts the set carries (0: none)
    DevBuf docs, bitmap, rank_dir, tile_dir;
    uint64_t device_bytes = 0;
    float ms_mark = -1.0f, ms_count_scan = -1.0f, ms_expand = -1.0f;  // VQ_DOCSET_TIMING=1: HIP event times of the three stages of its construction
    int route = -1;                // combine_docsets: 0 the word route built it, 1 the probe route; -1: no combine made it
    int range_route = -1;          // make_docset_from_ranges: 0 the stream route built it, 1 the probe route; -1: not made from ranges
    int device = 0;                // the index's GPU and the stream the set was built on (its index's: vq_docset_ids copies on it)
    hipStream_t stream = nullptr;
};
// The image from a filled scratch bitmap: `mark` queues on `st` whatever sets bit `doc` of the zeroed scratch bitmap over all anchors (and may count
// into meta[0] what it refused); count -> scan -> expand -> tiles follow.  len is the popcount of the whole scratch bitmap.  n: the ids of the
// caller's array, for the message about the refused ones
using DocSetMarkFn = std::function<void(hipStream_t st, uint32_t* scratch, uint64_t scratch_words, unsigned long long* meta)>;
std::shared_ptr<DocSet> docset_from_marks(const Index& idx, hipStream_t st, uint64_t n, const DocSetMarkFn& mark);
inline uint64_t docset_scratch_words(const Index& idx) { return ((uint64_t(idx.num_anchors) + 511u) / 512u) * 16u; }  // the whole anchor range, in whole 512-doc blocks
// ids: n anchor ids in any order, duplicates allowed, in host memory or (on_device) in the index's GPU's memory.  Synchronous.  An id >= num_anchors:
// ERR_INVALID_ARGUMENT, with their number in the message
std::shared_ptr<const DocSet> make_docset(const Index& idx, const uint32_t* ids, uint64_t n, bool on_device);
// The set of the docs a compiled filter selects: the presence-only postfix program fops over lists, both staged on the device (docset_filter.hip fills
// the scratch bitmap, the rest is make_docset's).  Synchronous, on `st`.  On a shard len is summed over the shards (Index::sum_over_shards)
std::shared_ptr<const DocSet> make_docset_from_program(const Index& idx, hipStream_t st, const DList* lists, uint32_t n_lists, const DOp* fops, uint32_t n_fops,
                                                       uint32_t stack_depth);
// Set algebra over staged sets of `idx` (docset_algebra.cpp, docset_algebra.hip): op 0 and, 1 or, 2 minus (sets[0] without the others), 3 not
// (n == 1: the anchors of [doc_lo, doc_hi) outside the set).  Any n >= 1.  Synchronous; each call owns its scratch, operands are only read.
// On a shard len is summed over the shards (Index::sum_over_shards)
enum { SETOP_AND = 0, SETOP_OR = 1, SETOP_MINUS = 2, SETOP_NOT = 3 };
std::shared_ptr<const DocSet> combine_docsets(const Index& idx, int op, const std::vector<std::shared_ptr<const DocSet>>& sets);
// The set of the docs whose column values satisfy every clause (docset_ranges.cpp, docset_ranges.hip).  A clause names the column
// "<field>.boost_valid_to_value" — anchor-keyed, or for a field with "[]" keyed by value id and joined to the anchors through
// "<field>.value_id_to_anchor" (a doc holds when any of its present values does) — and bounds it: a present, non-NaN f32 value v satisfies a bound b
// exactly when (double)v compares so to b; NaN satisfies nothing and counts as present; `missing`: a doc without a value satisfies the clause.
// `within` (null: none) is and-ed in.  Any number of clauses.  Synchronous; each call owns its scratch.  On a shard len is summed over the shards
// (Index::sum_over_shards), ERR_UNSUPPORTED without the hook
struct RangeClause {
    std::string field;
    bool has_lower = false, lower_open = false, has_upper = false, upper_open = false, missing = false;  // open: gt / lt
    double lower = 0.0, upper = 0.0;
};
// the clause list of vq_docset_from_ranges: throws vqjson::ParseError for a value of the wrong type, ERR_INVALID_ARGUMENT for a list or clause the
// interface refuses (empty list, no field, gt with gte, lt with lte, an unknown key)
std::vector<RangeClause> range_clauses_from_json(const vqjson::Value& v);
// [lo, hi] of range_key values a clause's bounds select, cut to [kRangeKeyMin, kRangeKeyMax]; lo > hi: nothing
void range_clause_keys(const RangeClause& c, uint32_t* lo, uint32_t* hi);
std::shared_ptr<const DocSet> make_docset_from_ranges(const Index& idx, const std::vector<RangeClause>& clauses, std::shared_ptr<const DocSet> within);
// The column "<field>.boost_valid_to_value" as the kernels take it (values, presence, key_base, num_keys; the rest of d zero) and, for a field
// with "[]", its "<field>.value_id_to_anchor" table (null: the column is keyed by doc).  make_docset_from_ranges and docset_aggregate share it:
// ERR_INVALID_ARGUMENT ("<what>: ... keyed by term ids") for a ".token_values" column, the search's ERR_INDEX_NOT_FOUND for an unknown column or a
// 1:n field without its table
struct RangeColumn {
    RangeClauseD d;
    const KVStore* to_anchor = nullptr;
};
RangeColumn resolve_range_column(const Index& idx, const std::string& field, const char* what);
float f32_at_or_above(double b);  // the smallest f32 (infinities included) that is >= b (no NaN)

// Numeric aggregations of a staged set (docset_aggs.cpp, docset_aggs.hip): per spec the set's docs (docs = DocSet::len), the present non-NaN values
// (count), the docs without a value (missing), the NaNs (nan), min / max compared through range_key (a zero is +0.0; 0 when count == 0), the exact
// sum of the finite counted values rounded once to f64 (+-inf / NaN by the infinities counted, 0.0 when nothing is), and with `edges` the
// len(edges) + 1 bucket counts: bucket b holds the values with exactly b edges e for which (double)v >= e.  Synchronous, on pre_stream (else
// stream); each call owns its state.  On a shard counters, buckets and limbs are summed in one call of Index::sum_over_shards, min / max agreed
// in four more (one-hot digit histograms of the keys' bytes, most significant first); ERR_UNSUPPORTED without the hook
struct AggSpec {
    std::string field;
    bool has_edges = false;
    std::vector<double> edges;
};
struct AggResult {
    uint64_t docs = 0, count = 0, missing = 0, nan = 0;
    double sum = 0.0;
    float min = 0.0f, max = 0.0f;
    std::vector<uint64_t> buckets;  // empty: the spec had no `edges`
};
// the spec list of vq_docset_aggregate: throws vqjson::ParseError for a value of the wrong type, ERR_INVALID_ARGUMENT for an empty list, a spec
// without `field`, an unknown key, more than kAggMaxEdges edges or edges that do not strictly ascend
std::vector<AggSpec> agg_specs_from_json(const vqjson::Value& v);
std::vector<AggResult> docset_aggregate(const Index& idx, const DocSet& ds, const std::vector<AggSpec>& specs);
// (pos - neg) * 2^-149 rounded once to f64, ties to even: pos / neg are 9 slots each, slot i weighs 2^(32 i) and may hold any u64 (carries are
// propagated here)
double agg_limbs_to_double(const uint64_t* pos, const uint64_t* neg);
// VQ_DOCSET_TIMING=1: the HIP event time (ms) of the kernels of this thread's last docset_aggregate; negative: none was launched or timed
float docset_aggregate_last_ms();
// A staged set ordered by a column (docset_top.cpp, docset_top.hip): rows [skip, skip + top) of the set's docs in the order (sort key ascending,
// doc ascending).  The sort key (kernels.hpp): range_key of the value (descending: its complement), kTopNanKey for a NaN, kTopMissingKey for a doc
// without a value; a 1:n doc gets the smallest sort key of its present values — so both directions list numbers, then NaN docs, then missing
// docs, ties by ascending doc id.  with_missing false: only docs with a number.  top + skip <= kTopMaxRows, else ERR_UNSUPPORTED.  Synchronous, on
// pre_stream (else stream); each call owns its scratch (4 B per local id, and for a 1:n field 4 B per doc of the index's doc range).  On a
// sharded index the result is the shard's part: its own first top + skip rows with skip not applied, its local counters, partial = true; no hook
// is called.  docset_top_merge puts parts together on the host
struct TopSpec {
    std::string field;
    uint32_t top = 10, skip = 0;
    bool descending = false, with_missing = true;
};
struct TopResult {
    TopSpec spec;
    bool partial = false;
    std::vector<uint32_t> docs, keys;  // the rows: doc and sort key
    std::vector<float> values;         // value_of_key for a number (a zero is +0.0), NaN for a NaN doc, 0.0 for a missing one
    std::vector<uint8_t> kinds;        // 0 number, 1 NaN, 2 missing
    uint64_t n_docs = 0, count = 0, nan = 0, missing = 0;  // in docs of the local set (a merge: of all parts); n_docs = count + nan + missing
};
// the spec of vq_docset_top_by: throws vqjson::ParseError for a value of the wrong type, ERR_INVALID_ARGUMENT for a spec without `field`, an
// unknown key or a top / skip that is no unsigned 32-bit integer
TopSpec top_spec_from_json(const vqjson::Value& v);
TopResult docset_top(const Index& idx, const DocSet& ds, const TopSpec& spec);
// host only: the parts of one call on every shard -> the whole index's page.  ERR_INVALID_ARGUMENT for no part, a null part, a part that is not
// partial beside others, parts whose top, skip, direction, with_missing or field differ
TopResult docset_top_merge(const std::vector<const TopResult*>& parts);
// a result as a flat byte image (a fixed header, the field, the rows as (sort key, doc) pairs) and back; unpack validates every length and the
// order of the rows and throws ERR_INVALID_ARGUMENT for a malformed image
std::vector<uint8_t> docset_top_pack(const TopResult& r);
TopResult docset_top_unpack(const uint8_t* bytes, size_t len);
// VQ_DOCSET_TIMING=1: the HIP event time (ms) of the kernels of this thread's last docset_top; negative: none was launched or timed
float docset_top_last_ms();
// The set's local ids (sorted, unique, unpadded): min(local_len, cap) of them to `out`, host memory or (on_device) memory of the set's GPU — then
// device to device on the set's stream, finished on return.  Returns local_len
uint64_t copy_docset_ids(const DocSet& ds, uint32_t* out, uint64_t cap, bool on_device);

// ------------------------------------------------------------------ compiled query
struct HList {
    const uint32_t* d_docs = nullptr;
    const uint16_t* d_scores = nullptr;
    uint32_t len = 0;
    uint32_t flags = 0;
    float term_score = 0.f;
    uint16_t max_raw = 0x7C00;  // +inf: no bound known
    uint16_t pivot_raw = 0x7C00;  // PostingStore::pivot_raw (== max_raw: the list has no score class)
    float max_value = std::numeric_limits<float>::infinity();  // LIST_F32 (materialised leaf): its largest value
    uint64_t global_len = 0;
    const uint32_t* d_bitmap = nullptr;
    const uint32_t* d_rank_dir = nullptr;
    const uint32_t* d_tile_dir = nullptr;
    const uint32_t* d_cov32 = nullptr;  // tile-packed image (PostingStore::cov32 / arr16 / gdir), null without one
    const uint16_t* d_arr16 = nullptr;
    const uint32_t* d_gdir = nullptr;
    uint32_t tile_most = 0;  // most 8-entry granules of the list in one 32768-doc tile (PostingStore::tile_most)
    int inline_idx = -1;  // >= 0: docs come from inline_lists[inline_idx] (carried inside the blob)
    int inline_val_idx = -1;  // >= 0: f32 values come from inline_vals[inline_val_idx]
};

struct FacetOut {
    std::string field;
    std::string dict_path;  // fst used to turn value ids into strings
    uint32_t top = 10;
    uint32_t num_values = 0;
    uint32_t host_top = 0;  // > 0: more entries than k_facet_select ranks (kMaxTopK) — the job's histogram is downloaded and ranked on the host; `top` is 0 then
};
// One FacetRequest resolved against the index (compile.cpp): the steps to the anchor, the direct / anchor_to_text_id / composed store, the histogram's
// length, top against kMaxTopK.  A search's facet stage and docset_facets share it, errors and declines included (f.hist_off / f.out_off: the caller's)
struct ResolvedFacet {
    DFacet f;
    FacetOut out;
};
ResolvedFacet resolve_facet(const Index& idx, const vqreq::FacetRequest& fr);

// ---- explain (src/search/result/explain.rs:2-21)
struct ExplainRec {
    enum Kind : uint8_t { Boost, MaxTokenToTextId, TermToAnchor, LevenshteinScore, OrSumOverDistinctTerms } kind = Boost;
    float a = 0.0f, b = 0.0f, c = 0.0f;  // Boost(a) | TermToAnchor{term_score a, anchor_score b, final_score c} | LevenshteinScore{score a} | OrSum(a)
    uint32_t term_id = 0;
    std::string text;  // LevenshteinScore.text_or_token_id
};
using ExplainRecs = std::vector<ExplainRec>;
struct ExplainNode {  // one node of the request's score tree, as the reference executes it (no leaf fusion, no materialised unions)
    uint32_t kind = 0;               // XP_LEAF / XP_AND / XP_OR
    int op = -1;                     // its op in ExplainPlan::ops
    std::vector<int> children;       // request order
    std::vector<uint16_t> order;     // AND: the operands in summation order (set_op.rs:393), the shortest one last
    // leaf: one list per matched term, in the order of the dictionary result's hits (search_field.rs:419)
    uint32_t list_begin = 0, list_count = 0;
    std::vector<uint32_t> list_term;
    std::map<uint32_t, ExplainRecs> term_records;  // the dictionary result's explain map, keyed by TERM id (search_field.rs:336-343; field_result.rs:44 copies it
                                                   // into the anchor-keyed result: an anchor whose id is one of these keys starts with that term's records)
};
using WhyFoundPlan = std::map<std::string, std::vector<uint32_t>>;
struct ExplainPlan {
    std::vector<ExplainNode> nodes;
    int root = -1;
    std::vector<ExList> lists;
    std::vector<ExOp> ops;
    std::vector<uint16_t> aux;
    std::vector<DColBoost> cols;  // the request-level column boosts (boost.rs:470-504), request order
};

struct CompiledQuery {
    size_t blob_bytes = 0, desc_bytes = 0;  // size of the packed blob / of its descriptor part, taken right after compilation on the compiling thread (0: not taken)
    int status = 0;
    std::shared_ptr<const ExplainPlan> explain_plan;  // request.explain: what complete_explain_requests needs for the returned hits
    // request.why_found with request.select (search.rs:220-224): textindex path -> all term ids the search matched there (what get_why_found flattens out of
    // term_id_hits_in_field, why_found.rs:24-27); complete_why_found_requests highlights the returned anchors' texts with them
    std::shared_ptr<const WhyFoundPlan> why_found_plan;
    std::shared_ptr<const DocSet> docset;  // the request's doc set: its lists point into the set's buffers, so the batch keeps it alive too
    std::string error;
    std::vector<RangeJob> range_requests;  // status == kStatusNeedsRanges
    std::vector<UnionJob> union_requests;  // status == kStatusNeedsUnion: jobs to run before compiling again
    std::vector<LocalityJob> locality_requests;  // likewise (K7)
    std::vector<Boost1nJob> boost1n_requests;    // likewise (K10)
    std::vector<uint32_t> count_nodes;     // status == kStatusNeedsCounts: node ids; counters 2i / 2i+1 = hits / hits inside the filter, then the filter
    uint32_t n_counts = 0;
    std::vector<HList> lists;
    std::vector<std::vector<uint32_t>> inline_lists;
    std::vector<std::vector<float>> inline_vals;
    std::vector<DColBoost> leaf_cols;  // compile-time staging of the OP_BOOST1N parameters
    uint32_t seq_tiles = 0;          // see QHeader::seq_tiles
    uint32_t prune_n = 0;            // see QHeader::prune_n
    uint64_t prune_mask = 0;
    uint32_t prune_gbits[16] = {};
    uint32_t n_top_cols = 0;  // cols[0 .. n_top_cols) are the request-level boosts; the rest belong to OP_BOOST1N ops
    std::vector<DOp> ops, fops;
    std::vector<DPresOp> pres;
    std::vector<uint16_t> pres_in;
    uint32_t n_temps = 0;
    uint32_t simple_n = 0;
    uint32_t simple_flags = 0;          // QHeader::simple_flags (the kSf* fields, device_types.hpp)
    KernelId kclass = K_TILE_SCAN;      // the scan kernel the query runs on (route_query, set once simple_flags is final)
    std::vector<DGroup> groups;
    std::vector<DTermBoost> tboosts;
    std::vector<DColBoost> cols;
    std::vector<DLocField> locf;
    std::vector<uint16_t> loc_idx;
    DSimple2 simple2{};  // kSfRich
    DWide wide{};        // kSfWide
    DProbe probe{};      // kSfProbe, kSfUnionPacked
    uint32_t probe_arr_gran = 0;  // ... the most granules any of its array operands has in one tile (the launch sizes the operands' LDS slot by it)
    std::vector<DFacet> facets;
    std::vector<FacetOut> facet_out;
    std::map<std::string, std::vector<std::string>> why_found_terms;  // search.rs:186: path -> matched term texts (request.why_found)
    uint32_t top = 10, skip = 0, top_k = 10;
    uint64_t total_len = 0;       // sum of shard-local list lengths (work estimate)
    uint64_t algorithmic_bytes = 0;
    uint64_t layout_bytes = 0;   // static part of KernelProfile::layout_bytes for this query (set when the kernel route is known)
    uint64_t key_upper = ~0ull;  // QHeader::key_upper
    // k_scan_probe_or (kSfProbeOr) scores only the docs that hold the cover; a doc without it scores at most this (the OR formula on the
    // other operands' list maxima).  The finished request is exact if its k-th best key lies above: finish_batch checks and otherwise asks for a
    // second run without the short cut (Result::rerun_exact).  NaN: not such a query.
    float or_skip_bound = std::numeric_limits<float>::quiet_NaN();
    bool deep = false;           // top + skip > kMaxTopK: this compilation ranks the first kMaxTopK only; the caller pages on (search_pages)
    uint32_t tile_words = 0, n_spans = 1, stack_depth = 1;
    uint32_t max_spans = 1;  // tiles of the query's doc range (<= 4096): a small batch splits its queries further, up to this (exec.cpp)
};

KernelId route_query(const CompiledQuery& cq);
// What the pre-passes of a batch have found so far, as one compilation pass sees it.  Null and non-null differ: the compiler asks for a union /
// range / locality job where it has no table and reads the job's result where it has one (exec.cpp: BatchTables hands these out per pass).
struct CompileInputs {
    const FuzzyTable* fuzzy = nullptr;
    const UnionTable* unions = nullptr;
    const QueryCounts* counts = nullptr;
    const RangeTable* ranges = nullptr;
    Boost1nCache* boost_cache = nullptr;
    const LocalityTable* localities = nullptr;
    bool topn_probes = false;  // `fuzzy` may hold top-n probes (FuzzyProbe::top_n): only the batched suggest sets it, every other caller looks up by fuzzy_key alone
};
CompiledQuery compile_query(const Index& idx, const vqreq::Request& req, const CompileInputs& in = {});
void run_locality_jobs(const Index& idx, Workspace& ws, LocalityTable& table, hipStream_t st);
void run_boost1n_jobs(const Index& idx, Workspace& ws, Boost1nTable& table, hipStream_t st);
void run_range_jobs(const Index& idx, Workspace& ws, RangeTable& table, const UnionTable& unions, hipStream_t st);
// dense_min: a job with more lists takes the dense route (at most 64 x 64, what two levels of k_union take); negative: the shipped rule
// (VQ_UNION_DENSE_MIN, else 64 x 64)
void run_union_jobs(const Index& idx, Workspace& ws, UnionTable& table, hipStream_t st, int64_t dense_min = -1);
void debug_prepass(const Index& idx, const std::function<void(Workspace&, hipStream_t)>& body);  // exec.cpp: what vq_debug_*_lists run the drivers in
// vq_docset_from_filter (exec.cpp): the ids the compiler's filter of a request with `filter` and doc set `within` (null: none) selects, as a doc set.
// The tree is compiled as a filter and nothing else (Request::filter_only) behind the dictionary scans and job pre-passes a batch gives it; every
// decline and error is the one a search with this filter returns
std::shared_ptr<const DocSet> make_docset_from_filter(const Index& idx, const vqreq::SearchRequest& filter, std::shared_ptr<const DocSet> within);
// What the count pre-pass measured for one request of a batch (vq_debug_node_counts).  status: 0 = counted, kNodeCountsNone = the request needs no
// count pre-pass, otherwise the error code its search would return (`error`: the text)
constexpr int kNodeCountsNone = -1;
struct NodeCounts {
    int status = 0;
    std::string error;
    bool has_filter = false;
    uint64_t filter_count = 0;
    uint32_t n_spans = 0, tile_words = 0;  // what the count query was compiled with
    struct Node {
        uint32_t id;  // the compiler's preorder number of the node in search_req
        uint64_t hits, hits_in_filter;
    };
    std::vector<Node> nodes;
};
std::vector<NodeCounts> debug_node_counts(const Index& idx, const vqreq::Request* const* reqs, size_t n, bool summed);  // exec.cpp
struct Result;
// Deep requests (top + skip > kMaxTopK) of an unsharded batch: results[i] holds page 0; fetch the following pages (each one scan that
// ranks only keys below the previous page's last) and cut the requested window.
// explain records of the returned hits (k_explain + host formatting); requests without `explain` are left alone
void complete_explain_requests(const Index& idx, std::vector<std::unique_ptr<Result>>& results, std::vector<int>& status, std::vector<std::string>& errors);
// why_found_info of the returned hits (get_why_found, search/why_found.rs:11-50): host work over the host copies of the key-value stores and the
// dictionary, on the final window of ids; requests without `why_found` + `select` are left alone
void complete_why_found_requests(const Index& idx, std::vector<std::unique_ptr<Result>>& results, std::vector<int>& status, std::vector<std::string>& errors);
bool request_wants_explain(const vqreq::Request& req);
std::string explain_records_json(const ExplainRecs& records);
void complete_deep_requests(const Index& idx, const vqreq::Request* const* reqs, size_t n, std::vector<std::unique_ptr<Result>>& results,
                            std::vector<int>& status, std::vector<std::string>& errors);

// ------------------------------------------------------------------ results
struct ResultFacet {
    std::string field;
    std::vector<std::pair<std::string, uint64_t>> entries;
};
struct Result {
    uint64_t num_hits = 0;
    uint64_t execution_time_ns = 0;
    std::vector<uint32_t> ids;
    std::vector<float> scores;
    std::vector<ResultFacet> facets;
    bool has_facets = false;
    std::map<std::string, std::vector<std::string>> why_found_terms;
    std::shared_ptr<const ExplainPlan> explain_plan;
    std::shared_ptr<const WhyFoundPlan> why_found_plan;
    std::map<uint32_t, std::map<std::string, std::vector<std::string>>> why_found_info;  // search.rs:220-224: anchor -> field -> highlighted texts
    bool has_explain = false;
    std::vector<std::pair<bool, ExplainRecs>> explain;  // per returned hit: (the reference's map has an entry for the hit, its records) — search.rs:86,96
    bool deep = false;  // holds the first page of a deep request (see CompiledQuery::deep)
    bool rerun_exact = false;  // k_scan_probe_or's short cut could not be confirmed (CompiledQuery::or_skip_bound): finish_batch runs the request again
    mutable std::string json;
};

// The facet counts of a staged set (docset_facets.cpp, docset_facets.hip): every requested field's values counted over the set's docs, ranked and
// rendered as a search over exactly these docs reports them.  num_hits = ds.len, no hits; the fields in request order.  Synchronous, on the index's
// stream; each call owns its scratch, the set is only read: any number of threads may call on one set.  On a shard the local histograms are summed
// over the shards before ranking (Index::sum_over_shards; every rank calls in the same order), ERR_UNSUPPORTED without the hook
std::unique_ptr<Result> docset_facets(const Index& idx, const DocSet& ds, const std::vector<vqreq::FacetRequest>& facets);
// the last call's count kernel in ms (HIP events), recorded per thread when VQ_DOCSET_TIMING is set; negative: none was launched or timed
float docset_facets_last_count_ms();

struct PartialBatch {
    const Index* index = nullptr;
    Workspace* ws = nullptr;
    std::unique_lock<std::mutex> lock;    // holds the workspace until the batch is finished
    bool pinned_ws = false;               // ... a workspace the caller named (Workspace::pinned is ours to clear)
    std::vector<CompiledQuery> queries;   // status != 0: failed at compile time
    std::vector<uint32_t> slot;           // slot[i]: position of request i among the device queries, or UINT32_MAX
    std::vector<uint8_t> qclass;          // profiling: KernelId of the scan that serves device query q
    std::vector<FacetJob> facet_jobs;     // host copy of the facet jobs (histogram offsets of the ones ranked on the host)
    uint32_t nq_dev = 0;
    PartialLayout layout{};
    // device addresses inside the workspace
    const uint8_t* d_blobs = nullptr;
    const uint32_t* d_blob_off = nullptr;
    const FacetJob* d_facet_jobs = nullptr;
    uint8_t* d_partial = nullptr;
    hipStream_t scan_stream = nullptr;  // where the batch's upload, scans and span merge are queued (the index's scan stream unless the caller named another)
    uint32_t total_spans = 0;
    uint32_t n_facet_jobs = 0;
    uint32_t total_facet_out = 0;
    bool profiled = false;
    bool launched = false, finished = false;  // scans queued / results taken
    bool merge_launched = false;              // finish_batch phase 1 done (merge + download queued on the finish stream)
    std::chrono::steady_clock::time_point t0;
    void release_workspace();
    std::vector<const vqreq::Request*> reqs;  // the batch's requests as handed in (alive until the batch is finished: a request may have to run again)
    std::vector<std::shared_ptr<const vqreq::Request>> owners;  // ... by construction where the batch outlives the call that made it: the ABI layer
                                                                // shares the handles' requests here.  Empty for a batch that ends inside its call
    ~PartialBatch();  // a batch given up before its merge waits for its scans: the workspace (pinned staging, blobs) is handed on only when the device is done with it
};

std::unique_ptr<PartialBatch> run_partial(const Index& idx, const vqreq::Request* const* reqs, size_t n, int slot = -1, int64_t arena_offset = -1,
                                          hipStream_t scan_stream = nullptr);  // scan_stream null: the index's
void finish_batch(const Index& idx, PartialBatch& pb, const void* gathered_device, uint32_t num_shards, std::vector<std::unique_ptr<Result>>& out,
                  std::vector<int>& status, std::vector<std::string>& errors, size_t shard_stride = 0);  // shard_stride: bytes between the shards'
                                                                                                         // copies in `gathered_device` (0: the partial's own size)
// the two halves of finish_batch: queue merge + download on the finish stream (nothing is waited for) / wait for them and build the results
void finish_launch(const Index& idx, PartialBatch& pb, const void* gathered_device, uint32_t num_shards, size_t shard_stride = 0);

}  // namespace vq
