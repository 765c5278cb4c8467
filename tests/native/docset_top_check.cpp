// TEST INFRASTRUCTURE — a doc set ordered by a column under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by
// tests/test_docset_top_cpu.py): built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device layer
// (hip_stub*.cpp; with VQ_STUB_DICT_SCAN=1, which this program sets, hip_stub_docset_top.cpp answers the launchers on the host).  It drives
//   a. vq_docset_top_by through the C ABI on a small index — a column without presence, one with a presence bitmap and NaNs, a 1:n column with its
//      value_id_to_anchor table — over a short set, a set with a bitmap and the empty set, in both directions, with and without the missing docs,
//      pages inside and past the set, with the select forced and on a capped grid, against an order computed here by comparing floats;
//   b. spec parsing and every error path;
//   c. two shards: the parts, their merge, pack and unpack (truncated, oversized and altered images included), parts that differ;
//   d. four threads on one set.
// Everything is freed again.  Prints DOCSET_TOP_CHECK_OK.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../../include/veloci_amd.h"

#define CHECK(x)                                                                      \
    do {                                                                              \
        if (!(x)) {                                                                   \
            std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, vq_last_error()); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static const uint32_t kAnchors = 70003, kLo = 20001, kHi = 50000, kValues = 90001;
using Ids = std::vector<uint32_t>;
static std::vector<float> g_full, g_sparse, g_m;
static std::vector<uint8_t> g_sparse_present, g_m_present;
static std::vector<uint64_t> g_a_off;
static Ids g_a_vals;
static long g_calls = 0;

static float grid(uint32_t x) { return float(int((x * 2654435761u) >> 25) - 64) / 4.0f; }  // quarter steps in [-16, 16): many ties
static void make_columns() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (uint32_t d = 0; d < kAnchors; ++d) {
        g_full.push_back(grid(d));
        g_sparse.push_back(d % 401u == 7u ? nan : grid(d + 7777u));
        g_sparse_present.push_back(uint8_t((d / 37u) % 3u == 0 || d == kLo || d == kHi - 1));
    }
    g_full[100] = 0.0f, g_full[101] = -0.0f, g_full[30000] = inf, g_full[30001] = -inf, g_full[60000] = 1e-45f, g_full[60001] = nan;
    g_a_off.push_back(0);
    for (uint32_t v = 0; v < kValues; ++v) {
        g_m.push_back(v % 501u == 5u ? nan : grid(v + 99u));
        g_m_present.push_back(uint8_t(v % 7u != 3u));
        if (v % 11u != 0u) {
            g_a_vals.push_back(uint32_t((uint64_t(v) * 48271u) % kAnchors));
            if (v % 13u == 0u) g_a_vals.push_back((v * 3u) % kAnchors);
        }
        g_a_off.push_back(g_a_vals.size());
    }
}

static vq_index* build(uint32_t lo, uint32_t hi) {
    vq_index_builder* b = vq_index_builder_new(kAnchors, lo, hi);
    CHECK(b);
    const char* terms = "alpha";
    const uint64_t toff[2] = {0, 5};
    const Ids anchors = {1, 30500, 60000};
    const uint64_t off[2] = {0, 3};
    const Ids scores(anchors.size(), 10u);
    CHECK(vq_index_add_fst(b, "body.textindex", 1, reinterpret_cast<const uint8_t*>(terms), toff) == VQ_OK);
    CHECK(vq_index_add_token_to_anchor_score(b, "body.textindex.to_anchor_id_score", 1, off, anchors.data(), scores.data(), nullptr) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "body.textindex.text_id_to_anchor", 0, 1, off, anchors.data()) == VQ_OK);
    auto bits = [](const std::vector<float>& v, uint32_t a, uint32_t n) {
        Ids out(n);
        std::memcpy(out.data(), v.data() + a, size_t(n) * 4);
        return out;
    };
    CHECK(vq_index_add_boost(b, "full.boost_valid_to_value", lo, hi - lo, nullptr, bits(g_full, lo, hi - lo).data()) == VQ_OK);
    CHECK(vq_index_add_boost(b, "sparse.boost_valid_to_value", lo, hi - lo, g_sparse_present.data() + lo, bits(g_sparse, lo, hi - lo).data()) == VQ_OK);
    CHECK(vq_index_add_boost(b, "m[].v.boost_valid_to_value", 0, kValues, g_m_present.data(), bits(g_m, 0, kValues).data()) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "m[].v.value_id_to_anchor", 0, kValues, g_a_off.data(), g_a_vals.data()) == VQ_OK);
    CHECK(vq_index_add_boost(b, "orphan[].v.boost_valid_to_value", 0, 100, nullptr, bits(g_m, 0, 100).data()) == VQ_OK);
    vq_index* idx = nullptr;
    CHECK(vq_index_build(b, 0, &idx) == VQ_OK && idx);
    vq_index_builder_free(b);
    return idx;
}

struct Row {
    uint32_t doc;
    int kind;  // 0 number, 1 NaN, 2 missing
    float value;
};
static const char* kFields[3] = {"full", "sparse", "m[].v"};
// the whole set in the order, by float compares
static std::vector<Row> order_of(int field, const Ids& ids, bool descending) {
    std::vector<Row> rows;
    std::vector<int> kind(kAnchors, 2);
    std::vector<float> best(kAnchors, 0.0f);
    if (field == 2) {
        for (uint32_t v = 0; v < kValues; ++v) {
            if (!g_m_present[v] || g_a_off[v] == g_a_off[v + 1]) continue;
            const uint32_t a = g_a_vals[g_a_off[v]];
            const float x = g_m[v];
            if (x != x) {
                if (kind[a] == 2) kind[a] = 1;
            } else if (kind[a] != 0 || (descending ? x > best[a] : x < best[a])) {
                kind[a] = 0;
                best[a] = x;
            }
        }
    }
    for (uint32_t d : ids) {
        Row r{d, 2, 0.0f};
        if (field == 2) {
            r.kind = kind[d];
            r.value = best[d];
        } else if (field == 0 || g_sparse_present[d]) {
            const float x = field == 0 ? g_full[d] : g_sparse[d];
            r.kind = x != x ? 1 : 0;
            r.value = x;
        }
        rows.push_back(r);
    }
    std::stable_sort(rows.begin(), rows.end(), [&](const Row& a, const Row& b) {
        if (a.kind != b.kind) return a.kind < b.kind;
        if (a.kind == 0 && a.value != b.value) return descending ? a.value > b.value : a.value < b.value;
        return a.doc < b.doc;
    });
    return rows;
}
static std::string spec_of(int field, uint32_t top, uint32_t skip, bool descending, bool with_missing) {
    return std::string("{\"field\": \"") + kFields[field] + "\", \"top\": " + std::to_string(top) + ", \"skip\": " + std::to_string(skip) +
           ", \"descending\": " + (descending ? "true" : "false") + ", \"with_missing\": " + (with_missing ? "true" : "false") + "}";
}
static void hold(const vq_docset_top* t, std::vector<Row> rows, uint32_t top, uint32_t skip, bool with_missing) {
    uint64_t want_c[4] = {rows.size(), 0, 0, 0};
    for (const Row& r : rows) ++want_c[1 + r.kind];
    if (!with_missing) rows.resize(size_t(want_c[1]));
    const size_t lo = std::min<size_t>(skip, rows.size()), hi = std::min<size_t>(size_t(skip) + top, rows.size());
    CHECK(vq_docset_top_len(t) == hi - lo);
    const uint32_t* docs = vq_docset_top_docs(t);
    const float* values = vq_docset_top_values(t);
    const uint8_t* kinds = vq_docset_top_kinds(t);
    for (size_t i = lo; i < hi; ++i) {
        const Row& r = rows[i];
        float want = r.kind == 0 ? r.value + 0.0f : 0.0f;
        CHECK(docs[i - lo] == r.doc && kinds[i - lo] == r.kind);
        if (r.kind == 1) CHECK(values[i - lo] != values[i - lo]);
        else CHECK(std::memcmp(&values[i - lo], &want, 4) == 0);
    }
    uint64_t c[4];
    vq_docset_top_counters(t, c);
    CHECK(c[0] == want_c[0] && c[1] == want_c[1] && c[2] == want_c[2] && c[3] == want_c[3]);
}
static vq_docset_top* top_by(const vq_index* idx, const vq_docset* d, const std::string& spec) {
    vq_docset_top* out = nullptr;
    CHECK(vq_docset_top_by(idx, d, spec.c_str(), spec.size(), &out) == VQ_OK && out);
    ++g_calls;
    return out;
}
static std::vector<uint8_t> image_of(const vq_docset_top* t) {
    const size_t need = vq_docset_top_pack(t, nullptr, 0);
    CHECK(need >= 64);
    std::vector<uint8_t> image(need);
    CHECK(vq_docset_top_pack(t, image.data(), need - 1) == need);  // too small: nothing is written, the size is answered
    CHECK(vq_docset_top_pack(t, image.data(), need) == need);
    return image;
}

static void check_pages(const vq_index* whole, const std::vector<vq_docset*>& sets, const std::vector<Ids>& lists) {
    for (size_t s = 0; s < sets.size(); ++s)
        for (int field = 0; field < 3; ++field)
            for (int dir = 0; dir < 2; ++dir) {
                const std::vector<Row> rows = order_of(field, lists[s], dir != 0);
                const uint32_t n = uint32_t(rows.size());
                const uint32_t pages[][2] = {{1, 0}, {10, 5}, {n, 0}, {n + 7, 0}, {5, n}, {0, 0}, {7, n > 3 ? n - 3 : 0}, {40, n / 2}};
                for (const auto& p : pages)
                    for (int wm = 0; wm < 2; ++wm) {
                        if (uint64_t(p[0]) + p[1] > 65536) continue;
                        vq_docset_top* t = top_by(whole, sets[s], spec_of(field, p[0], p[1], dir != 0, wm != 0));
                        CHECK(!vq_docset_top_is_partial(t));
                        hold(t, rows, p[0], p[1], wm != 0);
                        vq_docset_top_free(t);
                    }
            }
}

static void check_errors(const vq_index* whole, const vq_index* other, const vq_docset* d) {
    vq_docset_top* out = nullptr;
    auto rc = [&](const vq_index* i, const vq_docset* s, const char* text) { return vq_docset_top_by(i, s, text, text ? std::strlen(text) : 0, &out); };
    for (const char* bad : {"{\"field\": \"full\"", "[1]", "{\"field\": \"full\", \"top\": \"3\"}", "{\"field\": \"full\", \"skip\": true}", "{\"field\": \"full\", \"descending\": 1}",
                            "{\"field\": \"full\", \"with_missing\": \"no\"}", "{\"field\": 3}"})
        CHECK(rc(whole, d, bad) == VQ_ERR_JSON && !out);
    for (const char* bad : {"{\"top\": 3}", "{\"field\": \"full\", \"order\": 1}", "{\"field\": \"full\", \"top\": -1}", "{\"field\": \"full\", \"top\": 1.5}",
                            "{\"field\": \"full\", \"skip\": 1e12}", "{\"field\": \"body.textindex.token_values\"}"})
        CHECK(rc(whole, d, bad) == VQ_ERR_INVALID_ARGUMENT && !out);
    CHECK(rc(whole, d, "{\"field\": \"full\", \"top\": 65537}") == VQ_ERR_UNSUPPORTED && !out && std::strstr(vq_last_error(), "65536"));
    CHECK(rc(whole, d, "{\"field\": \"full\", \"top\": 65530, \"skip\": 7}") == VQ_ERR_UNSUPPORTED && !out);
    CHECK(rc(whole, d, "{\"field\": \"nosuch\"}") == VQ_ERR_INDEX_NOT_FOUND && !out && std::strstr(vq_last_error(), "nosuch.boost_valid_to_value"));
    CHECK(rc(whole, d, "{\"field\": \"orphan[].v\"}") == VQ_ERR_INDEX_NOT_FOUND && !out && std::strstr(vq_last_error(), "orphan[].v.value_id_to_anchor"));
    CHECK(rc(nullptr, d, "{\"field\": \"full\"}") == VQ_ERR_INVALID_ARGUMENT && rc(whole, nullptr, "{\"field\": \"full\"}") == VQ_ERR_INVALID_ARGUMENT);
    CHECK(rc(whole, d, nullptr) == VQ_ERR_INVALID_ARGUMENT && vq_docset_top_by(whole, d, "{}", 2, nullptr) == VQ_ERR_INVALID_ARGUMENT);
    CHECK(rc(other, d, "{\"field\": \"full\"}") == VQ_ERR_INVALID_ARGUMENT && !out && std::strstr(vq_last_error(), "another index"));
    CHECK(rc(whole, d, "{\"field\": \"full\", \"top\": null, \"descending\": null}") == VQ_OK && out && vq_docset_top_len(out) == 10);
    vq_docset_top_free(out);
    uint64_t c[4] = {1, 1, 1, 1};
    vq_docset_top_counters(nullptr, c);
    vq_docset_top_counters(nullptr, nullptr);
    CHECK(!c[0] && !c[3] && vq_docset_top_len(nullptr) == 0 && !vq_docset_top_docs(nullptr) && !vq_docset_top_values(nullptr) && !vq_docset_top_kinds(nullptr));
    CHECK(!vq_docset_top_is_partial(nullptr) && vq_docset_top_pack(nullptr, nullptr, 0) == 0);
    vq_docset_top_free(nullptr);
}

static long check_shards(const std::vector<Ids>& lists) {
    long merges = 0;
    vq_index* shards[2] = {build(0, kLo), build(kLo, kAnchors)};  // no hook is set: a top-k is no sum
    for (const Ids& ids : lists) {
        vq_docset* sets[2] = {nullptr, nullptr};
        for (int r = 0; r < 2; ++r) CHECK(vq_docset_create(shards[r], ids.data(), ids.size(), 0, &sets[r]) == VQ_OK);
        for (int field = 0; field < 3; ++field)
            for (int dir = 0; dir < 2; ++dir)
                for (int wm = 0; wm < 2; ++wm) {
                    const uint32_t top = 25, skip = dir ? 11 : 0;
                    const std::string spec = spec_of(field, top, skip, dir != 0, wm != 0);
                    // (the shards hold `full` and `sparse` cut to their doc range, so the whole column is what both see together)
                    vq_docset_top* parts[2] = {top_by(shards[0], sets[0], spec), top_by(shards[1], sets[1], spec)};
                    CHECK(vq_docset_top_is_partial(parts[0]) && vq_docset_top_is_partial(parts[1]));
                    vq_docset_top* merged = nullptr;
                    CHECK(vq_docset_top_merge(parts, 2, &merged) == VQ_OK && merged && !vq_docset_top_is_partial(merged));
                    hold(merged, order_of(field, ids, dir != 0), top, skip, wm != 0);
                    // pack -> unpack -> merge: the same image as the direct merge
                    vq_docset_top* back[2] = {nullptr, nullptr};
                    for (int r = 0; r < 2; ++r) {
                        const std::vector<uint8_t> image = image_of(parts[r]);
                        CHECK(vq_docset_top_unpack(image.data(), image.size(), &back[r]) == VQ_OK && back[r]);
                        CHECK(image_of(back[r]) == image);
                    }
                    vq_docset_top* again = nullptr;
                    CHECK(vq_docset_top_merge(back, 2, &again) == VQ_OK && image_of(again) == image_of(merged));
                    merges += 2;
                    for (vq_docset_top* t : {parts[0], parts[1], back[0], back[1], merged, again}) vq_docset_top_free(t);
                }
        // parts that differ, null parts, no part
        vq_docset_top* a = top_by(shards[0], sets[0], spec_of(0, 10, 0, false, true));
        vq_docset_top* out = nullptr;
        for (const std::string& other : {spec_of(0, 11, 0, false, true), spec_of(0, 10, 1, false, true), spec_of(0, 10, 0, true, true), spec_of(0, 10, 0, false, false),
                                         spec_of(1, 10, 0, false, true)}) {
            vq_docset_top* b = top_by(shards[1], sets[1], other);
            const vq_docset_top* both[2] = {a, b};
            CHECK(vq_docset_top_merge(both, 2, &out) == VQ_ERR_INVALID_ARGUMENT && !out && std::strstr(vq_last_error(), "differ"));
            vq_docset_top_free(b);
        }
        const vq_docset_top* with_null[2] = {a, nullptr};
        CHECK(vq_docset_top_merge(with_null, 2, &out) == VQ_ERR_INVALID_ARGUMENT && !out);
        CHECK(vq_docset_top_merge(with_null, 0, &out) == VQ_ERR_INVALID_ARGUMENT && vq_docset_top_merge(nullptr, 1, &out) == VQ_ERR_INVALID_ARGUMENT);
        CHECK(vq_docset_top_merge(with_null, 1, nullptr) == VQ_ERR_INVALID_ARGUMENT);
        // malformed images: every truncation, an oversized one, altered header words, rows out of order
        const std::vector<uint8_t> image = image_of(a);
        for (size_t cut = 0; cut < image.size(); ++cut) {
            std::vector<uint8_t> part(image.begin(), image.begin() + cut);  // (its own allocation: a read past `cut` is reported)
            CHECK(vq_docset_top_unpack(part.data(), part.size(), &out) == VQ_ERR_INVALID_ARGUMENT && !out);
        }
        std::vector<uint8_t> longer = image;
        longer.push_back(0);
        CHECK(vq_docset_top_unpack(longer.data(), longer.size(), &out) == VQ_ERR_INVALID_ARGUMENT && !out);
        for (size_t word : {0u, 1u, 2u, 5u, 6u, 7u, 8u, 10u}) {  // magic, version, flags, rows, field length, pad, docs, count
            std::vector<uint8_t> bad = image;
            bad[4 * word + 3] ^= 0x40;
            CHECK(vq_docset_top_unpack(bad.data(), bad.size(), &out) == VQ_ERR_INVALID_ARGUMENT && !out);
        }
        if (vq_docset_top_len(a) >= 2) {
            std::vector<uint8_t> bad = image;
            std::swap_ranges(bad.end() - 16, bad.end() - 8, bad.end() - 8);
            CHECK(vq_docset_top_unpack(bad.data(), bad.size(), &out) == VQ_ERR_INVALID_ARGUMENT && !out && std::strstr(vq_last_error(), "ascend"));
        }
        CHECK(vq_docset_top_unpack(nullptr, 64, &out) == VQ_ERR_INVALID_ARGUMENT && vq_docset_top_unpack(image.data(), image.size(), nullptr) == VQ_ERR_INVALID_ARGUMENT);
        vq_docset_top_free(a);
        for (vq_docset* d : sets) vq_docset_free(d);
    }
    for (vq_index* s : shards) vq_index_free(s);
    return merges;
}

int main() {
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    unsetenv("VQ_TOP_MAX_GRID");
    unsetenv("VQ_TOP_FORCE_SELECT");
    make_columns();
    vq_index* whole = build(0, kAnchors);
    vq_index* other = build(0, kAnchors);
    std::vector<Ids> lists(4);
    for (uint32_t d = 0; d < kAnchors; d += 3) lists[0].push_back(d);  // carries a bitmap
    lists[0].insert(lists[0].end(), {100, 101, 30000, 30001, 60000, 60001});
    std::sort(lists[0].begin(), lists[0].end());
    lists[0].erase(std::unique(lists[0].begin(), lists[0].end()), lists[0].end());
    lists[1] = {7, 100, 101, 408, 30000, 30001, 41000, 60000, 60001, 69999};
    lists[3] = {60001};
    std::vector<vq_docset*> sets(lists.size(), nullptr);
    for (size_t s = 0; s < lists.size(); ++s) CHECK(vq_docset_create(whole, lists[s].data(), lists[s].size(), 0, &sets[s]) == VQ_OK && sets[s]);
    check_pages(whole, sets, lists);
    setenv("VQ_TOP_MAX_GRID", "3", 1);
    check_pages(whole, sets, lists);
    unsetenv("VQ_TOP_MAX_GRID");
    setenv("VQ_TOP_FORCE_SELECT", "1", 1);
    check_pages(whole, sets, lists);
    unsetenv("VQ_TOP_FORCE_SELECT");
    check_errors(whole, other, sets[1]);
    const long merges = check_shards({lists[0], lists[1], lists[2]});
    {
        std::vector<std::thread> threads;
        const std::vector<Row> rows = order_of(2, lists[0], true);
        for (int t = 0; t < 4; ++t)
            threads.emplace_back([&] {
                for (int k = 0; k < 3; ++k) {
                    const std::string spec = spec_of(2, 30, 1000, true, true);
                    vq_docset_top* out = nullptr;
                    if (vq_docset_top_by(whole, sets[0], spec.c_str(), spec.size(), &out) != VQ_OK || !out) std::abort();
                    hold(out, rows, 30, 1000, true);
                    vq_docset_top_free(out);
                }
            });
        for (std::thread& t : threads) t.join();
    }
    for (vq_docset* d : sets) vq_docset_free(d);
    vq_index_free(whole);
    vq_index_free(other);
    std::printf("DOCSET_TOP_CHECK_OK {\"calls\": %ld, \"merges\": %ld}\n", g_calls, merges);
    return 0;
}
