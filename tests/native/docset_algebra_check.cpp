// TEST INFRASTRUCTURE — the doc set algebra under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by
// tests/test_docset_algebra_cpu.py): built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device layer
// (hip_stub*.cpp; with VQ_STUB_DICT_SCAN=1, which this program sets, hip_stub_docset_algebra.cpp answers the launchers on the host).  It builds a
// small index and a shard of it through the C ABI and drives vq_docset_combine: both routes and VQ_NO_SETOP_PROBE flipped in-process, operand
// lists far longer than the launchers' table, results as operands, operands freed right after the call, the sharded length through the hook, the
// export with a cap, and every error path; the ids are held against std::set_* computed here.  Everything is freed again.  Prints
// DOCSET_ALGEBRA_CHECK_OK.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
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

static const uint32_t kAnchors = 200003, kLo = 70001, kHi = 150000;
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
static Ids without(const Ids& a, const Ids& b) {
    Ids out;
    std::set_difference(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out));
    return out;
}

static vq_index* build(uint32_t lo, uint32_t hi) {
    vq_index_builder* b = vq_index_builder_new(kAnchors, lo, hi);
    CHECK(b);
    const char* terms = "alpha";
    const uint64_t toff[2] = {0, 5};
    const Ids anchors = {1, 70500, 149000};
    const uint64_t off[2] = {0, 3};
    const Ids scores(anchors.size(), 10u);
    CHECK(vq_index_add_fst(b, "body.textindex", 1, reinterpret_cast<const uint8_t*>(terms), toff) == VQ_OK);
    CHECK(vq_index_add_token_to_anchor_score(b, "body.textindex.to_anchor_id_score", 1, off, anchors.data(), scores.data(), nullptr) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "body.textindex.text_id_to_anchor", 0, 1, off, anchors.data()) == VQ_OK);
    vq_index* idx = nullptr;
    CHECK(vq_index_build(b, 0, &idx) == VQ_OK && idx);
    vq_index_builder_free(b);
    return idx;
}

static uint64_t g_total = 0;  // what the shard's hook answers: the whole set's size
static int g_hook_calls = 0;
static int hook(void*, uint64_t* values, size_t n) {
    if (n != 1) return 1;
    values[0] = g_total;
    ++g_hook_calls;
    return 0;
}

struct Side {
    vq_index* idx;
    uint32_t lo, hi;
};
static int g_sets = 0, g_probe = 0, g_word = 0;

static vq_docset* staged(const Side& s, const Ids& ids) {
    vq_docset* d = nullptr;
    CHECK(vq_docset_create(s.idx, ids.data(), ids.size(), 0, &d) == VQ_OK && d && vq_debug_docset_route(d) == -1);
    return d;
}
static void holds(const Side& s, const vq_docset* d, const Ids& want) {
    Ids local;
    for (uint32_t x : want)
        if (x >= s.lo && x < s.hi) local.push_back(x);
    CHECK(vq_docset_len(d) == want.size() && vq_docset_local_len(d) == local.size());
    Ids got(local.size() + 4, 0xABABABABu);
    CHECK(vq_docset_ids(d, got.data(), got.size(), 0) == local.size());
    CHECK(std::equal(local.begin(), local.end(), got.begin()) && got[local.size()] == 0xABABABABu);
    CHECK(vq_debug_docset_part(d, 4, nullptr, 0) % 4 == 0);
}
// the combine, held against `want`; route: what the rule says; a probe-route case runs again under VQ_NO_SETOP_PROBE
static vq_docset* combined(const Side& s, int op, const std::vector<const vq_docset*>& sets, const Ids& want, int route) {
    g_total = want.size();
    vq_docset* d = nullptr;
    CHECK(vq_docset_combine(s.idx, op, sets.data(), sets.size(), &d) == VQ_OK && d);
    CHECK(vq_debug_docset_route(d) == route);
    holds(s, d, want);
    ++g_sets;
    ++(route ? g_probe : g_word);
    if (route) {
        setenv("VQ_NO_SETOP_PROBE", "1", 1);
        vq_docset* w = nullptr;
        CHECK(vq_docset_combine(s.idx, op, sets.data(), sets.size(), &w) == VQ_OK && w && vq_debug_docset_route(w) == 0);
        unsetenv("VQ_NO_SETOP_PROBE");
        holds(s, w, want);
        CHECK(vq_docset_device_bytes(w) == vq_docset_device_bytes(d));
        vq_docset_free(w);
        ++g_sets;
    }
    return d;
}

int main() {
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    setenv("VQ_HOST_THREADS", "2", 1);
    unsetenv("VQ_NO_SETOP_PROBE");
    const Side whole{build(0, kAnchors), 0, kAnchors}, shard{build(kLo, kHi), kLo, kHi};
    const Ids thirds = every(3, 0), fifths = every(5, 2), all = every(1, 0);  // with a bitmap
    const Ids few = {0, 31, 32, 70000, 70001, 70002, 70005, 99999, 149999, 150000, kAnchors - 1};  // without
    const Ids rare = every(997, 70002);                                                              // without (131 ids)
    vq_docset* d = nullptr;
    {  // a shard without the hook declines, naming it; the whole index needs none
        vq_docset* a = staged(shard, thirds);
        const vq_docset* one[1] = {a};
        CHECK(vq_docset_combine(shard.idx, VQ_DOCSET_NOT, one, 1, &d) == VQ_ERR_UNSUPPORTED && !d && std::strstr(vq_last_error(), "vq_index_set_allreduce"));
        vq_docset_free(a);
    }
    CHECK(vq_index_set_allreduce(shard.idx, hook, nullptr) == VQ_OK);
    int on_shard = 0;
    for (const Side& s : {whole, shard}) {
        const int before = g_sets;
        vq_docset *a = staged(s, thirds), *b = staged(s, fifths), *f = staged(s, few), *r = staged(s, rare), *e = staged(s, Ids{});
        CHECK(vq_debug_docset_part(a, 1, nullptr, 0) && vq_debug_docset_part(b, 1, nullptr, 0) && !vq_debug_docset_part(f, 1, nullptr, 0) && !vq_debug_docset_part(r, 1, nullptr, 0));
        // pairs: every operation, operands with and without a bitmap on either side
        vq_docset_free(combined(s, VQ_DOCSET_AND, {a, b}, both(thirds, fifths), 0));
        vq_docset_free(combined(s, VQ_DOCSET_AND, {a, f}, both(thirds, few), 1));
        vq_docset_free(combined(s, VQ_DOCSET_AND, {r, f}, both(rare, few), 1));
        vq_docset_free(combined(s, VQ_DOCSET_AND, {a, e}, Ids{}, 1));
        vq_docset_free(combined(s, VQ_DOCSET_OR, {a, b}, any(thirds, fifths), 0));
        vq_docset_free(combined(s, VQ_DOCSET_OR, {f, a, r}, any(any(thirds, few), rare), 0));
        vq_docset_free(combined(s, VQ_DOCSET_OR, {f, r, e}, any(few, rare), 0));
        vq_docset_free(combined(s, VQ_DOCSET_MINUS, {a, b}, without(thirds, fifths), 0));
        vq_docset_free(combined(s, VQ_DOCSET_MINUS, {a, f, b, r}, without(without(without(thirds, few), fifths), rare), 0));
        vq_docset_free(combined(s, VQ_DOCSET_MINUS, {f, a}, without(few, thirds), 1));
        vq_docset_free(combined(s, VQ_DOCSET_MINUS, {f, r, a}, without(without(few, rare), thirds), 1));
        vq_docset_free(combined(s, VQ_DOCSET_NOT, {a}, without(all, thirds), 0));
        vq_docset_free(combined(s, VQ_DOCSET_NOT, {f}, without(all, few), 0));
        vq_docset_free(combined(s, VQ_DOCSET_NOT, {e}, all, 0));
        for (int op : {VQ_DOCSET_AND, VQ_DOCSET_OR, VQ_DOCSET_MINUS}) {  // one operand: a set equal to it
            vq_docset_free(combined(s, op, {a}, thirds, 0));
            vq_docset_free(combined(s, op, {f}, few, op == VQ_DOCSET_OR ? 0 : 1));
        }
        // far more operands than a launch takes: 70 sets that each lack 3 ids of their own, 70 small sets
        std::vector<vq_docset*> nearly, small;
        Ids lacking, small_union;
        for (uint32_t k = 0; k < 70; ++k) {
            const Ids hole = {k * 7u, 70001u + k * 11u, kAnchors - 1u - k};
            nearly.push_back(staged(s, without(all, hole)));
            lacking = any(lacking, hole);
            Ids some;
            for (uint32_t j = 0; j < 40; ++j) some.push_back((k * 2851u + j * 4999u) % kAnchors);
            std::sort(some.begin(), some.end());
            some.erase(std::unique(some.begin(), some.end()), some.end());
            small.push_back(staged(s, some));
            small_union = any(small_union, some);
        }
        std::vector<const vq_docset*> ops(nearly.begin(), nearly.end());
        vq_docset_free(combined(s, VQ_DOCSET_AND, ops, without(all, lacking), 0));
        ops.insert(ops.begin() + 33, f);
        vq_docset_free(combined(s, VQ_DOCSET_AND, ops, without(few, lacking), 1));  // the probe route in rounds
        ops.assign(small.begin(), small.end());
        vq_docset* u = combined(s, VQ_DOCSET_OR, ops, small_union, 0);
        ops.insert(ops.begin(), a);
        vq_docset_free(combined(s, VQ_DOCSET_MINUS, ops, without(thirds, small_union), 0));
        ops[0] = r;
        ops.insert(ops.end(), nearly.begin(), nearly.begin() + 20);  // 90 subtrahends, with and without a bitmap
        vq_docset_free(combined(s, VQ_DOCSET_MINUS, ops, without(without(rare, small_union), without(all, lacking)), 1));
        // a result as an operand; the operands freed right after the call
        vq_docset* x = combined(s, VQ_DOCSET_OR, {a, b}, any(thirds, fifths), 0);
        vq_docset* y = combined(s, VQ_DOCSET_MINUS, {x, u}, without(any(thirds, fifths), small_union), 0);
        vq_docset_free(x);
        vq_docset_free(u);
        holds(s, y, without(any(thirds, fifths), small_union));
        vq_docset* z = combined(s, VQ_DOCSET_NOT, {y}, without(all, without(any(thirds, fifths), small_union)), 0);
        vq_docset_free(y);
        holds(s, z, without(all, without(any(thirds, fifths), small_union)));
        // a result attached to a request compiles like any set
        const std::string text = "{\"search_req\":{\"search\":{\"path\":\"body\",\"terms\":[\"alpha\"]}}}";
        vq_request* req = nullptr;
        CHECK(vq_request_parse(text.data(), text.size(), &req) == VQ_OK && vq_request_set_docset(req, z) == VQ_OK);
        vq_docset_free(z);
        CHECK(vq_debug_compile(s.idx, req) == 0);
        vq_request_free(req);
        // the export with a cap
        uint32_t out[4] = {7, 7, 7, 7};
        CHECK(vq_docset_ids(r, out, 2, 0) == vq_docset_local_len(r) && out[0] == 70002u && out[1] == 70002u + 997u && out[2] == 7);
        CHECK(vq_docset_ids(e, nullptr, 0, 0) == 0 && vq_docset_ids(nullptr, out, 4, 0) == 0);
        // misuse
        const vq_docset* two[2] = {a, b};
        const vq_docset* holed[2] = {a, nullptr};
        CHECK(vq_docset_combine(s.idx, VQ_DOCSET_AND, two, 0, &d) == VQ_ERR_INVALID_ARGUMENT && !d);
        CHECK(vq_docset_combine(s.idx, VQ_DOCSET_AND, nullptr, 2, &d) == VQ_ERR_INVALID_ARGUMENT && !d);
        CHECK(vq_docset_combine(s.idx, VQ_DOCSET_OR, holed, 2, &d) == VQ_ERR_INVALID_ARGUMENT && !d);
        CHECK(vq_docset_combine(s.idx, 4, two, 2, &d) == VQ_ERR_INVALID_ARGUMENT && !d && vq_docset_combine(s.idx, -1, two, 2, &d) == VQ_ERR_INVALID_ARGUMENT);
        CHECK(vq_docset_combine(s.idx, VQ_DOCSET_NOT, two, 2, &d) == VQ_ERR_INVALID_ARGUMENT && !d);
        CHECK(vq_docset_combine(nullptr, VQ_DOCSET_AND, two, 2, &d) == VQ_ERR_INVALID_ARGUMENT && vq_docset_combine(s.idx, VQ_DOCSET_AND, two, 2, nullptr) == VQ_ERR_INVALID_ARGUMENT);
        const Side& other = s.lo ? whole : shard;
        CHECK(vq_docset_combine(other.idx, VQ_DOCSET_AND, two, 2, &d) == VQ_ERR_INVALID_ARGUMENT && !d && std::strstr(vq_last_error(), "another index"));
        for (vq_docset* p : nearly) vq_docset_free(p);
        for (vq_docset* p : small) vq_docset_free(p);
        for (vq_docset* p : {a, b, f, r, e}) vq_docset_free(p);
        if (s.lo) on_shard = g_sets - before;
    }
    CHECK(g_hook_calls == on_shard && on_shard * 2 == g_sets);  // one u64 per set combined on the shard, none on the whole index
    CHECK(vq_debug_docset_route(nullptr) == -1);
    vq_index_free(whole.idx);
    vq_index_free(shard.idx);
    std::printf("DOCSET_ALGEBRA_CHECK_OK {\"sets\": %d, \"probe\": %d, \"word\": %d}\n", g_sets, g_probe, g_word);
    return 0;
}
