// TEST INFRASTRUCTURE — doc sets under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by tests/test_docset_cpu.py):
// built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device layer (hip_stub*.cpp; with
// VQ_STUB_DICT_SCAN=1, which this program sets, hip_stub_docset.cpp answers the doc-set launchers on the host).  It builds a small index and a
// shard of it through the C ABI, creates sets (empty, sparse, dense, with duplicates, with foreign ids), reads their parts back, attaches them to
// requests, frees handle and request in both orders, compiles the requests against the right and the wrong index; everything is freed again.
// Prints DOCSET_CHECK_OK.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/veloci_amd.h"

#define CHECK(x)                                                                      \
    do {                                                                              \
        if (!(x)) {                                                                   \
            std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, vq_last_error()); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static const uint32_t kAnchors = 200003;

static vq_index* build(uint32_t lo, uint32_t hi) {
    vq_index_builder* b = vq_index_builder_new(kAnchors, lo, hi);
    CHECK(b);
    const char* terms = "alphabeta";
    const uint64_t toff[3] = {0, 5, 9}, off[3] = {0, 3, 5};
    const uint32_t anchors[5] = {1, 70500, 149000, 2, 100000}, scores[5] = {10, 10, 10, 10, 10};
    CHECK(vq_index_add_fst(b, "body.textindex", 2, reinterpret_cast<const uint8_t*>(terms), toff) == VQ_OK);
    CHECK(vq_index_add_token_to_anchor_score(b, "body.textindex.to_anchor_id_score", 2, off, anchors, scores, nullptr) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "body.textindex.text_id_to_anchor", 0, 2, off, anchors) == VQ_OK);
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

int main() {
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    setenv("VQ_HOST_THREADS", "2", 1);
    vq_index* whole = build(0, kAnchors);
    vq_index* shard = build(70001, 150000);
    int sets = 0;
    uint32_t seed = 12345;
    auto next = [&] { return seed = seed * 1664525u + 1013904223u; };
    for (vq_index* idx : {whole, shard}) {
        const uint32_t lo = idx == whole ? 0 : 70001, hi = idx == whole ? kAnchors : 150000;
        for (size_t n : {size_t(0), size_t(1), size_t(7), size_t(5000), size_t(90000)}) {
            std::vector<uint32_t> ids(n);
            for (auto& x : ids) x = next() % kAnchors;
            if (n > 3) ids[3] = ids[0];  // a duplicate
            std::set<uint32_t> uniq(ids.begin(), ids.end());
            std::vector<uint32_t> local;
            for (uint32_t x : uniq)
                if (x >= lo && x < hi) local.push_back(x);
            vq_docset* d = nullptr;
            CHECK(vq_docset_create(idx, ids.data(), ids.size(), 0, &d) == VQ_OK && d);
            CHECK(vq_docset_len(d) == uniq.size() && vq_docset_local_len(d) == local.size());
            std::vector<uint32_t> got(local.size() + 8, 0xABABABABu);
            CHECK(vq_debug_docset_part(d, 0, got.data(), got.size()) == local.size());
            CHECK(std::equal(local.begin(), local.end(), got.begin()) && got[local.size()] == 0xABABABABu);
            CHECK(vq_debug_docset_part(d, 0, got.data(), 1) == local.size());  // (a short buffer: the count, one element copied)
            const uint64_t padded = vq_debug_docset_part(d, 4, nullptr, 0);
            CHECK(padded == ((local.size() + 3) & ~size_t(3)));
            const uint64_t words = vq_debug_docset_part(d, 1, nullptr, 0), ranks = vq_debug_docset_part(d, 2, nullptr, 0);
            const bool dense = uint64_t(hi - lo) >= 65536 && local.size() * 64 >= uint64_t(hi - lo);
            CHECK((words != 0) == dense && (ranks != 0) == dense);
            if (dense) {
                std::vector<uint32_t> bm(words), rd(ranks);
                CHECK(vq_debug_docset_part(d, 1, bm.data(), words) == words && vq_debug_docset_part(d, 2, rd.data(), ranks) == ranks && ranks == words / 16 + 1);
                const uint32_t base = lo & ~65535u;
                uint64_t bits = 0;
                for (uint64_t w = 0; w < words; ++w) bits += uint64_t(__builtin_popcount(bm[w]));
                CHECK(bits == local.size() && rd[0] == 0 && rd[ranks - 1] == local.size());
                for (uint32_t x : local) CHECK((bm[(x - base) >> 5] >> ((x - base) & 31u)) & 1u);
            }
            CHECK(vq_docset_device_bytes(d) >= padded * 4);
            CHECK(vq_debug_docset_part(d, 9, nullptr, 0) == 0);
            float t[3];
            CHECK(vq_debug_docset_timings(d, t, t + 1, t + 2) == -1);
            vq_docset_free(d);
            ++sets;
        }
        // foreign ids: refused, nothing leaks
        const uint32_t bad[4] = {5, kAnchors, 9, 0xFFFFFFFFu};
        vq_docset* d = nullptr;
        CHECK(vq_docset_create(idx, bad, 4, 0, &d) == VQ_ERR_INVALID_ARGUMENT && !d && std::strstr(vq_last_error(), "2 of the 4 ids"));
        CHECK(vq_docset_create(idx, nullptr, 3, 0, &d) == VQ_ERR_INVALID_ARGUMENT && vq_docset_create(nullptr, bad, 1, 0, &d) == VQ_ERR_INVALID_ARGUMENT);
    }
    // attach, free in both orders, compile
    const std::string plain = "{\"search_req\":{\"search\":{\"path\":\"body\",\"terms\":[\"alpha\"]}}}";
    const std::string own = "{\"search_req\":{\"search\":{\"path\":\"body\",\"terms\":[\"alpha\"]}},\"filter\":{\"search\":{\"path\":\"body\",\"terms\":[\"beta\"]}}}";
    const std::string and3 = "{\"search_req\":{\"and\":{\"queries\":[{\"search\":{\"path\":\"body\",\"terms\":[\"alpha\"]}},{\"search\":{\"path\":\"body\",\"terms\":[\"beta\"]}},"
                             "{\"search\":{\"path\":\"body\",\"terms\":[\"alpha\"]}}]}}}";
    int compiled = 0;
    for (const std::string& text : {plain, own}) {
        const uint32_t ids[5] = {100000, 1, 2, 1, 149000};
        vq_docset* d = nullptr;
        CHECK(vq_docset_create(whole, ids, 5, 0, &d) == VQ_OK);
        vq_request* r1 = parse(text);
        vq_request* r2 = parse(text);
        const std::string before = vq_request_to_json(r1);
        CHECK(vq_request_set_docset(r1, d) == VQ_OK && vq_request_set_docset(r2, d) == VQ_OK);
        CHECK(before == vq_request_to_json(r1));
        CHECK(vq_debug_compile(whole, r1) == 0);
        vq_request_free(r2);  // a request first ...
        vq_docset_free(d);    // ... then the handle: r1 keeps the set
        CHECK(vq_debug_compile(whole, r1) == 0);
        CHECK(vq_debug_compile(shard, r1) == VQ_ERR_INVALID_ARGUMENT);  // the set belongs to `whole`
        vq_request* page = nullptr;
        CHECK(vq_request_page_after(r1, 1.0f, 7, &page) == VQ_OK);  // a continuation carries the set
        CHECK(vq_debug_compile(shard, page) == VQ_ERR_INVALID_ARGUMENT && vq_debug_compile(whole, page) == 0);
        CHECK(vq_request_set_docset(r1, nullptr) == VQ_OK && vq_debug_compile(shard, r1) == 0);
        vq_request_free(r1);
        CHECK(vq_debug_compile(whole, page) == 0);  // (r1 is gone: the page holds the set on its own)
        vq_request_free(page);
        CHECK(vq_request_set_docset(nullptr, nullptr) == VQ_ERR_INVALID_ARGUMENT);
        compiled += 1;
    }
    {  // an empty set; a 3-term AND under a set waits for the count pre-pass like one under a filter
        vq_docset *none = nullptr, *two = nullptr;
        const uint32_t ids[2] = {1, 2};
        CHECK(vq_docset_create(whole, nullptr, 0, 0, &none) == VQ_OK && vq_docset_len(none) == 0);
        CHECK(vq_docset_create(whole, ids, 2, 0, &two) == VQ_OK);
        vq_request* r = parse(and3);
        CHECK(vq_debug_compile(whole, r) == 0);
        CHECK(vq_request_set_docset(r, none) == VQ_OK && vq_debug_compile(whole, r) == -2);
        CHECK(vq_request_set_docset(r, two) == VQ_OK && vq_debug_compile(whole, r) == -2);
        vq_docset_free(none);
        vq_docset_free(two);
        vq_request_free(r);
    }
    vq_docset_free(nullptr);
    vq_index_free(whole);
    vq_index_free(shard);
    std::printf("DOCSET_CHECK_OK {\"sets\": %d, \"compiled\": %d}\n", sets, compiled);
    return 0;
}
