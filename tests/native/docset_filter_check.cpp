// TEST INFRASTRUCTURE — doc sets from a filter under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by
// tests/test_docset_filter_cpu.py): built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device layer
// (hip_stub*.cpp; with VQ_STUB_DICT_SCAN=1, which this program sets, hip_stub_docset_filter.cpp answers the launcher on the host).  It builds a small
// index and a shard of it through the C ABI, makes sets from a leaf, from a tree and within another set, holds their ids against sets computed
// here, frees the three handles in every order, and walks the error paths; everything is freed again.  Prints DOCSET_FILTER_CHECK_OK.
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
using Ids = std::vector<uint32_t>;

static Ids every(uint32_t step, uint32_t from) {
    Ids out;
    for (uint32_t d = from; d < kAnchors; d += step) out.push_back(d);
    return out;
}
static Ids both(const Ids& a, const Ids& b) {
    Ids out;
    std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out));
    return out;
}
static Ids any(const Ids& a, const Ids& b) {
    Ids out;
    std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out));
    return out;
}

// alpha: every 3rd doc (a dense list), beta: every 5th, gamma: a handful around the shard's borders
static const Ids kAlpha = every(3, 0), kBeta = every(5, 2), kGamma = {0, 70000, 70001, 70002, 99999, 149999, 150000, kAnchors - 1};

static vq_index* build(uint32_t lo, uint32_t hi) {
    vq_index_builder* b = vq_index_builder_new(kAnchors, lo, hi);
    CHECK(b);
    const char* terms = "alphabetagamma";
    const uint64_t toff[4] = {0, 5, 9, 14};
    Ids anchors;
    std::vector<uint64_t> off{0};
    for (const Ids* l : {&kAlpha, &kBeta, &kGamma}) {
        anchors.insert(anchors.end(), l->begin(), l->end());
        off.push_back(anchors.size());
    }
    const Ids scores(anchors.size(), 10u);
    CHECK(vq_index_add_fst(b, "body.textindex", 3, reinterpret_cast<const uint8_t*>(terms), toff) == VQ_OK);
    CHECK(vq_index_add_token_to_anchor_score(b, "body.textindex.to_anchor_id_score", 3, off.data(), anchors.data(), scores.data(), nullptr) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "body.textindex.text_id_to_anchor", 0, 3, off.data(), anchors.data()) == VQ_OK);
    vq_index* idx = nullptr;
    CHECK(vq_index_build(b, 0, &idx) == VQ_OK && idx);
    vq_index_builder_free(b);
    return idx;
}

static std::string leaf(const char* term) { return std::string("{\"search\":{\"path\":\"body\",\"terms\":[\"") + term + "\"]}}"; }

static uint64_t g_total = 0;  // what the shard's hook answers: the whole set's size
static int g_hook_calls = 0;
static int hook(void*, uint64_t* values, size_t n) {
    if (n != 1) return 1;
    values[0] = g_total;
    ++g_hook_calls;
    return 0;
}

static vq_docset* make(vq_index* idx, const std::string& filter, const vq_docset* within, const Ids& want, uint32_t lo, uint32_t hi) {
    g_total = want.size();
    vq_docset* d = nullptr;
    CHECK(vq_docset_from_filter(idx, filter.data(), filter.size(), within, &d) == VQ_OK && d);
    Ids local;
    for (uint32_t x : want)
        if (x >= lo && x < hi) local.push_back(x);
    CHECK(vq_docset_len(d) == want.size() && vq_docset_local_len(d) == local.size());
    Ids got(local.size() + 4, 0xABABABABu);
    CHECK(vq_debug_docset_part(d, 0, got.data(), got.size()) == local.size());
    CHECK(std::equal(local.begin(), local.end(), got.begin()) && got[local.size()] == 0xABABABABu);
    return d;
}

int main() {
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    setenv("VQ_HOST_THREADS", "2", 1);
    vq_index* whole = build(0, kAnchors);
    vq_index* shard = build(70001, 150000);
    const std::string f_leaf = leaf("alpha");
    const std::string f_tree = "{\"and\":{\"queries\":[" + leaf("alpha") + ",{\"or\":{\"queries\":[" + leaf("beta") + "," + leaf("gamma") + "," + leaf("nosuch") + "]}}]}}";
    const Ids w_leaf = kAlpha, w_tree = both(kAlpha, any(kBeta, kGamma)), w_within = both(kBeta, w_tree);
    CHECK(!w_within.empty() && w_within.size() < w_tree.size());
    int sets = 0, orders = 0;
    vq_docset* d = nullptr;
    // a shard without the hook declines, naming it
    CHECK(vq_docset_from_filter(shard, f_leaf.data(), f_leaf.size(), nullptr, &d) == VQ_ERR_UNSUPPORTED && !d && std::strstr(vq_last_error(), "vq_index_set_allreduce"));
    CHECK(vq_index_set_allreduce(shard, hook, nullptr) == VQ_OK);
    for (vq_index* idx : {whole, shard}) {
        const uint32_t lo = idx == whole ? 0 : 70001, hi = idx == whole ? kAnchors : 150000;
        int order[3] = {0, 1, 2};
        do {  // from a leaf, from a tree within it, from a leaf within that: freed in every order, the later sets read after the earlier are gone
            vq_docset* s[3];
            s[0] = make(idx, f_leaf, nullptr, w_leaf, lo, hi);
            s[1] = make(idx, f_tree, s[0], w_tree, lo, hi);
            s[2] = make(idx, leaf("beta"), s[1], w_within, lo, hi);
            sets += 3;
            for (int k = 0; k < 3; ++k) {
                vq_docset_free(s[order[k]]);
                s[order[k]] = nullptr;
                for (int j = 0; j < 3; ++j)
                    if (s[j]) CHECK(vq_docset_len(s[j]) == (j == 0 ? w_leaf.size() : j == 1 ? w_tree.size() : w_within.size()) && vq_debug_docset_part(s[j], 4, nullptr, 0) % 4 == 0);
            }
            ++orders;
        } while (std::next_permutation(order, order + 3));
        // a set from a filter restricts a request like any other
        vq_docset* ds = make(idx, f_tree, nullptr, w_tree, lo, hi);
        const std::string text = "{\"search_req\":" + leaf("alpha") + "}";
        vq_request* r = nullptr;
        CHECK(vq_request_parse(text.data(), text.size(), &r) == VQ_OK && vq_request_set_docset(r, ds) == VQ_OK);
        vq_docset_free(ds);
        CHECK(vq_debug_compile(idx, r) == 0);
        vq_request_free(r);
        ++sets;
        // an unknown term alone: the empty set; an empty and: the same
        vq_docset* none = make(idx, leaf("nosuch"), nullptr, Ids{}, lo, hi);
        vq_docset* within_none = make(idx, f_leaf, none, Ids{}, lo, hi);
        vq_docset_free(none);
        vq_docset_free(within_none);
        vq_docset_free(make(idx, "{\"and\":{\"queries\":[]}}", nullptr, Ids{}, lo, hi));
        sets += 3;
    }
    CHECK(g_hook_calls == sets / 2);  // one u64 per set made on the shard
    // misuse
    vq_docset* of_whole = make(whole, f_leaf, nullptr, w_leaf, 0, kAnchors);
    CHECK(vq_docset_from_filter(shard, f_leaf.data(), f_leaf.size(), of_whole, &d) == VQ_ERR_INVALID_ARGUMENT && !d);
    vq_docset_free(of_whole);
    const std::string broken = "{\"search\":{\"path\":", nopath = "{\"search\":{\"path\":\"nofield\",\"terms\":[\"x\"]}}";
    CHECK(vq_docset_from_filter(whole, broken.data(), broken.size(), nullptr, &d) == VQ_ERR_JSON && !d);
    CHECK(vq_docset_from_filter(whole, nopath.data(), nopath.size(), nullptr, &d) == VQ_ERR_FST_NOT_FOUND && !d && std::strstr(vq_last_error(), "nofield"));
    CHECK(vq_docset_from_filter(nullptr, f_leaf.data(), f_leaf.size(), nullptr, &d) == VQ_ERR_INVALID_ARGUMENT);
    CHECK(vq_docset_from_filter(whole, nullptr, 0, nullptr, &d) == VQ_ERR_INVALID_ARGUMENT && vq_docset_from_filter(whole, f_leaf.data(), f_leaf.size(), nullptr, nullptr) == VQ_ERR_INVALID_ARGUMENT);
    vq_index_free(whole);
    vq_index_free(shard);
    std::printf("DOCSET_FILTER_CHECK_OK {\"sets\": %d, \"orders\": %d}\n", sets + 1, orders);
    return 0;
}
