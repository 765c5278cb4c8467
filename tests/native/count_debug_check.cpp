// TEST INFRASTRUCTURE — vq_debug_node_counts (capi.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by
// tests/test_count_debug_cpu.py): built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device layer
// (hip_stub*.cpp).  With VQ_STUB_NOOP_LAUNCH=1, which this program sets, the launchers return without doing anything and "device" memory is zeroed
// host memory: the count pre-pass runs to its end over counters nobody added to, so the compilation passes in front of it, the packing of the
// count queries, the per-query counter offsets of a batch and the copy-out are walked and every number that comes back is 0 (VQ_STUB_DICT_SCAN=1
// lets the stub build the doc sets on the host).  Then the arguments the function must refuse (-2) and a failing launch (-1).
// Prints COUNT_DEBUG_CHECK_OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/veloci_amd.h"

extern "C" void vq_stub_fail_launches_after(long k);

#define CHECK(x)                                                                                      \
    do {                                                                                              \
        if (!(x)) {                                                                                   \
            std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, vq_last_error()); \
            std::exit(1);                                                                             \
        }                                                                                             \
    } while (0)

static const uint32_t kAnchors = 200003;

static vq_index* build() {
    vq_index_builder* b = vq_index_builder_new(kAnchors, 0, kAnchors);
    CHECK(b);
    const char* terms = "alphabetagamma";
    const uint64_t toff[4] = {0, 5, 9, 14}, off[4] = {0, 3, 5, 9};
    const uint32_t anchors[9] = {1, 70500, 149000, 2, 100000, 1, 2, 70500, 200002}, scores[9] = {10, 10, 10, 10, 10, 10, 10, 10, 10};
    CHECK(vq_index_add_fst(b, "body.textindex", 3, reinterpret_cast<const uint8_t*>(terms), toff) == VQ_OK);
    CHECK(vq_index_add_token_to_anchor_score(b, "body.textindex.to_anchor_id_score", 3, off, anchors, scores, nullptr) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "body.textindex.text_id_to_anchor", 0, 3, off, anchors) == VQ_OK);
    CHECK(vq_index_set_column_meta(b, "body", 0, 1) == VQ_OK);
    vq_index* idx = nullptr;
    CHECK(vq_index_build(b, 0, &idx) == VQ_OK && idx);
    vq_index_builder_free(b);
    return idx;
}

static vq_request* parse(const std::string& json) {
    vq_request* r = nullptr;
    CHECK(vq_request_parse(json.data(), json.size(), &r) == VQ_OK && r);
    return r;
}

struct Out {
    std::vector<int> status;
    std::vector<uint32_t> has_filter, n_spans, tile_words, node_ids;
    std::vector<uint64_t> filter_count, node_off, hits, inside;
    Out(size_t n, size_t cap)
        : status(n, 77), has_filter(n, 77), n_spans(n, 77), tile_words(n, 77), node_ids(cap + 1, 77), filter_count(n, 77), node_off(n + 1, 77), hits(cap + 1, 77), inside(cap + 1, 77) {}
};
static int call(const vq_index* idx, const std::vector<const vq_request*>& reqs, int summed, uint64_t cap, Out& o) {
    return vq_debug_node_counts(idx, reqs.data(), reqs.size(), summed, cap, o.status.data(), o.has_filter.data(), o.filter_count.data(), o.n_spans.data(), o.tile_words.data(),
                                o.node_off.data(), o.node_ids.data(), o.hits.data(), o.inside.data());
}

int main() {
    setenv("VQ_STUB_NOOP_LAUNCH", "1", 1);
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    setenv("VQ_HOST_THREADS", "2", 1);
    vq_index* idx = build();
    vq_index* other = build();
    CHECK(vq_profile_enable(idx, 1) == VQ_OK);
    const std::string leaves = "{\"search\":{\"path\":\"body\",\"terms\":[\"alpha\"]}},{\"search\":{\"path\":\"body\",\"terms\":[\"beta\"]}},{\"search\":{\"path\":\"body\",\"terms\":[\"gamma\"]}}";
    const std::string and3 = "{\"search_req\":{\"and\":{\"queries\":[" + leaves + "]}}}";
    const std::string and3_filter = "{\"search_req\":{\"and\":{\"queries\":[" + leaves + "]}},\"filter\":{\"search\":{\"path\":\"body\",\"terms\":[\"gamma\"]}}}";
    const std::string nested = "{\"search_req\":{\"and\":{\"queries\":[{\"or\":{\"queries\":[" + leaves + "]}}," + leaves + "]}},\"filter\":{\"search\":{\"path\":\"body\",\"terms\":[\"beta\"]}}}";
    vq_request *plain = parse(and3), *filtered = parse(and3_filter), *with_set = parse(and3), *foreign = parse(and3), *deep = parse(nested);
    const uint32_t ids[4] = {1, 2, 70500, 1};
    vq_docset *set = nullptr, *set_other = nullptr;
    CHECK(vq_docset_create(idx, ids, 4, 0, &set) == VQ_OK && vq_docset_create(other, ids, 4, 0, &set_other) == VQ_OK);
    CHECK(vq_request_set_docset(with_set, set) == VQ_OK && vq_request_set_docset(foreign, set_other) == VQ_OK);
    size_t ok = 0, refused = 0;

    {  // a request that needs no count pre-pass: nothing is measured, no array for the nodes is needed
        Out o(1, 0);
        CHECK(vq_debug_node_counts(idx, &plain, 1, 1, 0, o.status.data(), o.has_filter.data(), o.filter_count.data(), o.n_spans.data(), o.tile_words.data(), o.node_off.data(),
                                   nullptr, nullptr, nullptr) == 0);
        CHECK(o.status[0] == VQ_COUNTS_NONE && o.node_off[0] == 0 && o.node_off[1] == 0 && o.n_spans[0] == 0 && o.tile_words[0] == 0 && o.has_filter[0] == 0);
        CHECK(!std::strstr(vq_profile_json(idx, 1), "k_tile_scan<count pre-pass>"));  // nothing was launched
        ++ok;
    }
    for (const vq_request* r : {(const vq_request*)filtered, (const vq_request*)with_set}) {  // a counted one, alone: the three operands are nodes 1, 2, 3
        for (int summed = 0; summed <= 1; ++summed) {
            Out o(1, 3);
            CHECK(call(idx, {r}, summed, 3, o) == 0);
            CHECK(o.status[0] == VQ_OK && o.has_filter[0] == 1 && o.filter_count[0] == 0 && o.n_spans[0] >= 1 && o.tile_words[0] >= 64);
            CHECK(o.node_off[0] == 0 && o.node_off[1] == 3 && o.node_ids[0] == 1 && o.node_ids[1] == 2 && o.node_ids[2] == 3 && o.node_ids[3] == 77);
            CHECK(o.hits[0] == 0 && o.hits[2] == 0 && o.hits[3] == 77 && o.inside[2] == 0 && o.inside[3] == 77);  // (the launcher added nothing) and nothing beyond the nodes
            ++ok;
        }
    }
    CHECK(std::strstr(vq_profile_json(idx, 1), "k_tile_scan<count pre-pass>"));
    {  // a batch that interleaves counted, uncounted and failing requests
        const std::vector<const vq_request*> reqs = {plain, filtered, nullptr, deep, foreign, with_set, plain};
        Out o(reqs.size(), 16);
        CHECK(call(idx, reqs, 1, 16, o) == 0);
        const int want[7] = {VQ_COUNTS_NONE, VQ_OK, VQ_ERR_INVALID_ARGUMENT, VQ_OK, VQ_ERR_INVALID_ARGUMENT, VQ_OK, VQ_COUNTS_NONE};
        const uint64_t off[8] = {0, 0, 3, 3, 7, 7, 10, 10};
        for (size_t i = 0; i < reqs.size(); ++i) CHECK(o.status[i] == want[i] && o.node_off[i] == off[i]);
        CHECK(o.node_off[7] == 10 && std::strstr(vq_last_error(), "null request"));
        const uint32_t ids_want[10] = {1, 2, 3, 1, 5, 6, 7, 1, 2, 3};  // (deep: the OR is node 1, its leaves 2 - 4, the AND's own leaves 5 - 7)
        for (size_t k = 0; k < 10; ++k) CHECK(o.node_ids[k] == ids_want[k] && o.hits[k] == 0 && o.inside[k] == 0);
        CHECK(o.node_ids[10] == 77 && o.has_filter[3] == 1 && o.has_filter[0] == 0 && o.tile_words[2] == 0);
        CHECK(call(idx, reqs, 1, 10, o) == 0);
        CHECK(call(idx, reqs, 1, 9, o) == -2);  // capacity too small for the nodes
        ok += 2;
        ++refused;
    }
#define REFUSED(call_)        \
    do {                      \
        CHECK((call_) == -2); \
        ++refused;            \
    } while (0)
    {
        Out o(1, 3);
        const vq_request* one = filtered;
        REFUSED(call(nullptr, {filtered}, 1, 3, o));
        REFUSED(vq_debug_node_counts(idx, nullptr, 1, 1, 3, o.status.data(), o.has_filter.data(), o.filter_count.data(), o.n_spans.data(), o.tile_words.data(), o.node_off.data(),
                                     o.node_ids.data(), o.hits.data(), o.inside.data()));
        REFUSED(vq_debug_node_counts(idx, &one, 0, 1, 3, o.status.data(), o.has_filter.data(), o.filter_count.data(), o.n_spans.data(), o.tile_words.data(), o.node_off.data(),
                                     o.node_ids.data(), o.hits.data(), o.inside.data()));
        REFUSED(call(idx, {filtered}, 2, 3, o));
        REFUSED(call(idx, {filtered}, -1, 3, o));
        REFUSED(vq_debug_node_counts(idx, &one, 1, 1, 3, nullptr, o.has_filter.data(), o.filter_count.data(), o.n_spans.data(), o.tile_words.data(), o.node_off.data(),
                                     o.node_ids.data(), o.hits.data(), o.inside.data()));
        REFUSED(vq_debug_node_counts(idx, &one, 1, 1, 3, o.status.data(), o.has_filter.data(), o.filter_count.data(), o.n_spans.data(), o.tile_words.data(), nullptr,
                                     o.node_ids.data(), o.hits.data(), o.inside.data()));
        REFUSED(vq_debug_node_counts(idx, &one, 1, 1, 3, o.status.data(), o.has_filter.data(), o.filter_count.data(), o.n_spans.data(), o.tile_words.data(), o.node_off.data(),
                                     o.node_ids.data(), nullptr, o.inside.data()));
        REFUSED(call(idx, {filtered}, 1, 2, o));
        // an unknown doc set — one made for another index: the request's own error, as from the search; the call itself ran
        CHECK(call(idx, {foreign}, 1, 3, o) == 0 && o.status[0] == VQ_ERR_INVALID_ARGUMENT && o.node_off[1] == 0 && std::strstr(vq_last_error(), "another index"));
        ++ok;
    }
    // a launch that fails: -1, and the index stays usable
    {
        Out o(1, 3);
        vq_stub_fail_launches_after(0);
        CHECK(call(idx, {filtered}, 1, 3, o) == -1 && std::strstr(vq_last_error(), "injected failure"));
        vq_stub_fail_launches_after(-1);
        CHECK(call(idx, {filtered}, 1, 3, o) == 0 && o.status[0] == VQ_OK);
        ++ok;
    }
    for (vq_request* r : {plain, filtered, with_set, foreign, deep}) vq_request_free(r);
    vq_docset_free(set);
    vq_docset_free(set_other);
    vq_index_free(idx);
    vq_index_free(other);
    std::printf("COUNT_DEBUG_CHECK_OK {\"ok\": %zu, \"refused\": %zu}\n", ok, refused);
    return 0;
}
