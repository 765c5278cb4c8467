// TEST INFRASTRUCTURE — the doc sets from numeric ranges under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by
// tests/test_docset_ranges_cpu.py): built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device layer
// (hip_stub*.cpp; with VQ_STUB_DICT_SCAN=1, which this program sets, hip_stub_docset_ranges.cpp answers the launchers on the host).  It builds a
// small index and a shard of it through the C ABI — a column without presence, one with a presence bitmap, one that begins and ends inside the doc
// range at an odd key_base, a 1:n column with its value_id_to_anchor table — and drives vq_docset_from_ranges: every bound kind with bounds at
// stored values, at 0.1 against float32(0.1), at the zeros, below the denormals and at the infinities, `missing`, 9 and 17 clauses, 1:n clauses,
// both routes with VQ_NO_RANGE_PROBE flipped in-process, the sum over the shards through the hook, four threads on a shared `within`, and every
// error path; the ids are held against a comparison in double computed here.  Everything is freed again.  Prints DOCSET_RANGES_CHECK_OK.
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

static const uint32_t kAnchors = 200003, kLo = 70001, kHi = 150000, kLateShift = 1003, kLateKeys = 50001, kValues = 260001;
using Ids = std::vector<uint32_t>;

struct Bound {
    bool on = false, open = false;
    double b = 0.0;
};
struct Clause {
    int field;  // 0 full, 1 sparse, 2 late, 3 m[].v
    Bound lower, upper;
    bool missing;
    std::string text;  // the bounds as they go into the JSON
};
static const char* const kFields[4] = {"full", "sparse", "late", "m[].v"};

static std::vector<float> g_full, g_sparse, g_late, g_m;
static std::vector<uint8_t> g_sparse_present, g_m_present;
static std::vector<uint64_t> g_a_off;
static Ids g_a_vals;

static float grid(uint32_t x) { return float(int((x * 2654435761u) >> 19) - 4096) / 4.0f; }  // quarter steps in [-1024, 1024)
static void make_columns() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float specials[12] = {0.0f, -0.0f, inf, -inf, nan, 1e-45f, -1e-45f, 0.1f, 16777216.0f, 16777218.0f, std::numeric_limits<float>::max(), -std::numeric_limits<float>::max()};
    for (uint32_t d = 0; d < kAnchors; ++d) {
        g_full.push_back(grid(d));
        g_sparse.push_back(grid(d + 7777u));
        g_late.push_back(grid(d + 31u));
        g_sparse_present.push_back(uint8_t((d / 37u) % 3u == 0 || d == kLo || d == kHi - 1));  // runs of 37 docs
    }
    for (uint32_t base : {40u, kLo + 2000u, kHi - 40u, 180000u})
        for (uint32_t k = 0; k < 12; ++k) {
            g_full[base + k] = g_sparse[base + k] = g_late[base + k] = specials[k];
            g_sparse_present[base + k] = 1;
        }
    // value ids -> anchors, not monotone; every 11th row is empty, every 13th holds a second entry that counts for nothing
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

static bool inside(float v, const Clause& c) {
    if (v != v) return false;
    const double x = double(v);
    if (c.lower.on && !(c.lower.open ? x > c.lower.b : x >= c.lower.b)) return false;
    if (c.upper.on && !(c.upper.open ? x < c.upper.b : x <= c.upper.b)) return false;
    return true;
}
// per clause the docs that hold, on the index of [lo, hi) (`late` sits at lo + kLateShift)
static std::vector<uint8_t> holds(const Clause& c, uint32_t lo) {
    std::vector<uint8_t> ok(kAnchors, 0);
    if (c.field == 3) {
        std::vector<uint8_t> has(kAnchors, 0);
        for (uint32_t v = 0; v < kValues; ++v) {
            if (!g_m_present[v] || g_a_off[v] == g_a_off[v + 1]) continue;
            const uint32_t a = g_a_vals[g_a_off[v]];
            has[a] = 1;
            if (inside(g_m[v], c)) ok[a] = 1;
        }
        for (uint32_t d = 0; d < kAnchors; ++d)
            if (c.missing && !has[d]) ok[d] = 1;
        return ok;
    }
    for (uint32_t d = 0; d < kAnchors; ++d) {
        bool present = true;
        float v = g_full[d];
        if (c.field == 1) present = g_sparse_present[d], v = g_sparse[d];
        if (c.field == 2) present = d >= lo + kLateShift && d < lo + kLateShift + kLateKeys, v = g_late[d];
        ok[d] = present ? inside(v, c) : c.missing;
    }
    return ok;
}

static std::string number(double b) {
    if (std::isinf(b)) return b > 0 ? "1e999" : "-1e999";
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.17g", b);
    return buf;
}
static Clause clause(int field, const char* lower_key, double lower, const char* upper_key, double upper, bool missing) {
    Clause c{field, {}, {}, missing, ""};
    c.text = std::string("{\"field\":\"") + kFields[field] + "\"";
    if (lower_key) {
        c.lower = Bound{true, std::strcmp(lower_key, "gt") == 0, lower};
        c.text += std::string(",\"") + lower_key + "\":" + number(lower);
    }
    if (upper_key) {
        c.upper = Bound{true, std::strcmp(upper_key, "lt") == 0, upper};
        c.text += std::string(",\"") + upper_key + "\":" + number(upper);
    }
    c.text += missing ? ",\"missing\":true}" : "}";
    return c;
}
static std::string json_of(const std::vector<Clause>& cs) {
    std::string s = "[";
    for (size_t i = 0; i < cs.size(); ++i) s += (i ? "," : "") + cs[i].text;
    return s + "]";
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
    auto bits = [](const std::vector<float>& v, uint32_t a, uint32_t n) {
        Ids out(n);
        std::memcpy(out.data(), v.data() + a, size_t(n) * 4);
        return out;
    };
    CHECK(vq_index_add_boost(b, "full.boost_valid_to_value", lo, hi - lo, nullptr, bits(g_full, lo, hi - lo).data()) == VQ_OK);
    CHECK(vq_index_add_boost(b, "sparse.boost_valid_to_value", lo, hi - lo, g_sparse_present.data() + lo, bits(g_sparse, lo, hi - lo).data()) == VQ_OK);
    CHECK(vq_index_add_boost(b, "late.boost_valid_to_value", lo + kLateShift, kLateKeys, nullptr, bits(g_late, lo + kLateShift, kLateKeys).data()) == VQ_OK);
    CHECK(vq_index_add_boost(b, "m[].v.boost_valid_to_value", 0, kValues, g_m_present.data(), bits(g_m, 0, kValues).data()) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "m[].v.value_id_to_anchor", 0, kValues, g_a_off.data(), g_a_vals.data()) == VQ_OK);
    CHECK(vq_index_add_boost(b, "orphan[].v.boost_valid_to_value", 0, 100, nullptr, bits(g_m, 0, 100).data()) == VQ_OK);
    vq_index* idx = nullptr;
    CHECK(vq_index_build(b, 0, &idx) == VQ_OK && idx);
    vq_index_builder_free(b);
    return idx;
}

static uint64_t g_local = 0, g_total = 0;
static int g_hook_calls = 0, g_hook_bad = 0;
static int hook(void*, uint64_t* values, size_t n) {
    ++g_hook_calls;
    if (n != 1 || values[0] != g_local) {
        ++g_hook_bad;
        return 1;
    }
    values[0] = g_total;
    return 0;
}

struct Side {
    vq_index* idx;
    uint32_t lo, hi;
};
static int g_sets = 0, g_probe = 0;
static uint64_t g_ids = 0;

// the set of `cs` under `within` (null: none; within_ids its ids) against the comparison in double; route: the one the rule gives
static void check_set(const Side& s, const std::vector<Clause>& cs, const vq_docset* within, const Ids* within_ids, int route) {
    std::vector<uint8_t> ok(kAnchors, 1);
    for (const Clause& c : cs) {
        const std::vector<uint8_t> h = holds(c, s.lo);
        for (uint32_t d = 0; d < kAnchors; ++d) ok[d] &= h[d];
    }
    if (within_ids) {
        std::vector<uint8_t> in(kAnchors, 0);
        for (uint32_t d : *within_ids) in[d] = 1;
        for (uint32_t d = 0; d < kAnchors; ++d) ok[d] &= in[d];
    }
    Ids want;
    g_total = 0;
    for (uint32_t d = 0; d < kAnchors; ++d) {
        g_total += ok[d];
        if (ok[d] && d >= s.lo && d < s.hi) want.push_back(d);
    }
    g_local = want.size();
    const std::string text = json_of(cs);
    for (int forced = 0; forced < (route == 1 ? 2 : 1); ++forced) {
        if (forced) setenv("VQ_NO_RANGE_PROBE", "1", 1);
        vq_docset* d = nullptr;
        CHECK(vq_docset_from_ranges(s.idx, text.data(), text.size(), within, &d) == VQ_OK && d);
        if (forced) unsetenv("VQ_NO_RANGE_PROBE");
        CHECK(vq_debug_docset_range_route(d) == (forced ? 0 : route) && vq_debug_docset_route(d) == -1);
        CHECK(vq_docset_len(d) == g_total && vq_docset_local_len(d) == want.size());
        Ids got(want.size() + 1, 0xABCDu);
        CHECK(vq_docset_ids(d, got.data(), want.size(), 0) == want.size());
        got.pop_back();
        CHECK(got == want);
        vq_docset_free(d);
        ++g_sets;
        g_probe += !forced && route == 1;
        g_ids += want.size();
    }
}

int main() {
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    setenv("VQ_HOST_THREADS", "2", 1);
    unsetenv("VQ_NO_RANGE_PROBE");
    make_columns();
    const Side whole{build(0, kAnchors), 0, kAnchors}, shard{build(kLo, kHi), kLo, kHi};
    const double inf = std::numeric_limits<double>::infinity(), f32_01 = double(0.1f), flt_max = double(std::numeric_limits<float>::max());
    const double stored = double(grid(12345));
    std::vector<std::vector<Clause>> lists = {
        {clause(0, "gte", stored, nullptr, 0, false)}, {clause(0, "gt", stored, nullptr, 0, false)}, {clause(0, nullptr, 0, "lte", stored, false)}, {clause(0, nullptr, 0, "lt", stored, false)},
        {clause(0, "gte", -100.0, "lt", 100.25, false)}, {clause(1, "gt", -3.5, "lte", 7.75, false)},
        {clause(0, "gt", 0.05, "lte", 0.1, false)}, {clause(0, "gte", 0.1, "lt", 0.25, false)}, {clause(0, "gt", 0.05, "lte", f32_01, false)}, {clause(0, "gt", 0.05, "lt", f32_01, false)},
        {clause(0, "gte", 0.0, "lt", 0.25, false)}, {clause(0, "gt", 0.0, "lt", 0.25, false)}, {clause(0, "gt", -0.25, "lte", -0.0, false)}, {clause(0, "gt", -0.25, "lt", 0.0, false)},
        {clause(0, "gt", 1e-50, "lt", 0.25, false)}, {clause(0, "gt", -0.25, "lt", -1e-50, false)}, {clause(0, "gte", -1e-50, "lte", 1e-50, false)}, {clause(0, "gte", 1e-50, "lte", 2e-45, false)},
        {clause(0, "gte", inf, nullptr, 0, false)}, {clause(0, "gt", flt_max, nullptr, 0, false)}, {clause(1, nullptr, 0, "lte", -inf, false)}, {clause(0, "gt", -inf, "lt", inf, false)},
        {clause(0, "gt", inf, nullptr, 0, false)}, {clause(0, "gte", 1e300, nullptr, 0, false)}, {clause(0, "gt", 16777216.0, "lt", 16777218.0, false)}, {clause(0, "gte", 16777217.0, "lt", 2e7, false)},
        {clause(0, "gte", 5.0, "lte", 4.0, false)}, {clause(1, "gte", 5.0, "lte", 4.0, true)}, {clause(0, nullptr, 0, nullptr, 0, false)}, {clause(1, nullptr, 0, nullptr, 0, true)},
        {clause(1, "gte", 0.0, "lt", 500.0, true)}, {clause(2, "gte", -500.0, "lte", 500.0, false)}, {clause(2, "gt", 900.0, nullptr, 0, true)},
        {clause(0, "gte", -100.0, nullptr, 0, false), clause(0, nullptr, 0, "lt", 100.25, false)},
        {clause(3, "gte", 0.0, "lt", 50.0, false)}, {clause(3, "gte", 900.0, nullptr, 0, true)}, {clause(3, "gte", 5.0, "lte", 4.0, true)},
        {clause(0, "gte", -800.0, nullptr, 0, false), clause(3, nullptr, 0, "lt", 0.0, false), clause(1, "gte", -900.0, nullptr, 0, true)},
    };
    std::vector<Clause> many;
    for (int k = 0; k < 17; ++k) {
        many.push_back(k % 2 ? clause(k % 3, nullptr, 0, "lt", 990.0 - 7.25 * k, k % 3 != 0) : clause(k % 3, "gte", -990.0 + 6.5 * k, nullptr, 0, k % 3 != 0));
        if (k == 8 || k == 16) lists.push_back(many);
    }
    std::vector<Clause> with_1n(many.begin(), many.begin() + 8);
    with_1n.push_back(clause(3, nullptr, 0, "lt", 800.0, true));
    lists.push_back(with_1n);

    Ids dense, few;
    for (uint32_t d = 0; d < kAnchors; ++d) {
        if (d % 5 < 2) dense.push_back(d);
        if (d % 997 == 3 || d == 0 || d == 31 || d == kLo - 1 || d == kLo || d == kHi - 1 || d == kHi || d == kAnchors - 1 || (d >= kLo + 2000 && d < kLo + 2012)) few.push_back(d);
    }
    vq_docset* d = nullptr;
    {  // a shard without the hook declines, naming it
        const std::string text = json_of(lists[0]);
        CHECK(vq_docset_from_ranges(shard.idx, text.data(), text.size(), nullptr, &d) == VQ_ERR_UNSUPPORTED && !d && std::strstr(vq_last_error(), "vq_index_set_allreduce"));
    }
    CHECK(vq_index_set_allreduce(shard.idx, hook, nullptr) == VQ_OK);
    for (const Side& s : {whole, shard}) {
        const int hooks_before = g_hook_calls, sets_before = g_sets;
        vq_docset *w_dense = nullptr, *w_few = nullptr, *w_empty = nullptr;
        CHECK(vq_docset_create(s.idx, dense.data(), dense.size(), 0, &w_dense) == VQ_OK && vq_docset_create(s.idx, few.data(), few.size(), 0, &w_few) == VQ_OK);
        CHECK(vq_docset_create(s.idx, nullptr, 0, 0, &w_empty) == VQ_OK);
        const Ids none;
        for (const auto& cs : lists) {
            bool one_to_n = false;
            for (const Clause& c : cs) one_to_n = one_to_n || c.field == 3;
            check_set(s, cs, nullptr, nullptr, 0);
            check_set(s, cs, w_dense, &dense, 0);
            check_set(s, cs, w_few, &few, one_to_n ? 0 : 1);
            check_set(s, cs, w_empty, &none, one_to_n ? 0 : 1);
        }
        if (!s.lo) {  // four threads on a shared `within` (the whole index: the hook of the shard is one conversation)
            const std::string text = json_of(lists[4]);
            std::vector<uint8_t> ok = holds(lists[4][0], 0);
            Ids want;
            for (uint32_t x : few)
                if (ok[x]) want.push_back(x);
            std::vector<std::thread> pool;
            std::vector<int> good(4, 0);
            for (int t = 0; t < 4; ++t)
                pool.emplace_back([&, t] {
                    for (int k = 0; k < 3; ++k) {
                        vq_docset* q = nullptr;
                        if (vq_docset_from_ranges(s.idx, text.data(), text.size(), (t & 1) ? w_few : nullptr, &q) != VQ_OK || !q) return;
                        Ids got(kAnchors);
                        got.resize(vq_docset_ids(q, got.data(), got.size(), 0));
                        const bool same = (t & 1) ? got == want : got.size() == vq_docset_len(q) && got.size() > want.size();
                        vq_docset_free(q);
                        if (!same) return;
                    }
                    good[t] = 1;
                });
            for (auto& t : pool) t.join();
            CHECK(good == std::vector<int>(4, 1));
        }
        // misuse
        const Side& other = s.lo ? whole : shard;
        vq_docset* foreign = nullptr;
        CHECK(vq_docset_create(other.idx, few.data(), few.size(), 0, &foreign) == VQ_OK);
        const std::string fine = "[{\"field\":\"full\",\"gte\":1}]";
        CHECK(vq_docset_from_ranges(s.idx, fine.data(), fine.size(), foreign, &d) == VQ_ERR_INVALID_ARGUMENT && !d && std::strstr(vq_last_error(), "another index"));
        CHECK(vq_docset_from_ranges(nullptr, fine.data(), fine.size(), nullptr, &d) == VQ_ERR_INVALID_ARGUMENT && vq_docset_from_ranges(s.idx, nullptr, 0, nullptr, &d) == VQ_ERR_INVALID_ARGUMENT);
        CHECK(vq_docset_from_ranges(s.idx, fine.data(), fine.size(), nullptr, nullptr) == VQ_ERR_INVALID_ARGUMENT);
        for (const char* bad : {"[{\"field\":\"full\",\"gte\":1", "{\"field\":\"full\"}", "[{\"field\":\"full\",\"gte\":\"10\"}]", "[{\"field\":\"full\",\"lt\":true}]", "[{\"field\":\"full\",\"missing\":1}]",
                                "[{\"field\":7}]", "[3]", "[{\"field\":\"full\",\"gte\":1,\"gte\":2}]"})
            CHECK(vq_docset_from_ranges(s.idx, bad, std::strlen(bad), nullptr, &d) == VQ_ERR_JSON && !d);
        for (const char* bad : {"[]", "[{\"gte\":1}]", "[{\"field\":\"full\",\"gt\":1,\"gte\":1}]", "[{\"field\":\"full\",\"lt\":1,\"lte\":1}]", "[{\"field\":\"full\",\"ge\":1}]",
                                "[{\"field\":\"body.textindex.token_values\",\"gte\":1}]"})
            CHECK(vq_docset_from_ranges(s.idx, bad, std::strlen(bad), nullptr, &d) == VQ_ERR_INVALID_ARGUMENT && !d);
        const char* unknown = "[{\"field\":\"nosuch\",\"gte\":1}]";
        CHECK(vq_docset_from_ranges(s.idx, unknown, std::strlen(unknown), nullptr, &d) == VQ_ERR_INDEX_NOT_FOUND && !d &&
              std::strcmp(vq_last_error(), "Did not found path in indices nosuch.boost_valid_to_value") == 0);
        const char* orphan = "[{\"field\":\"orphan[].v\",\"gte\":1}]";
        CHECK(vq_docset_from_ranges(s.idx, orphan, std::strlen(orphan), nullptr, &d) == VQ_ERR_INDEX_NOT_FOUND && !d &&
              std::strcmp(vq_last_error(), "Did not found path in indices orphan[].v.value_id_to_anchor") == 0);
        for (vq_docset* x : {w_dense, w_few, w_empty, foreign}) vq_docset_free(x);
        if (s.lo) CHECK(g_hook_calls - hooks_before == g_sets - sets_before);  // the hook: once per set made on the shard
        else CHECK(g_hook_calls == hooks_before);                              // an unsharded index never calls it
    }
    CHECK(g_hook_bad == 0);
    vq_index_free(whole.idx);
    vq_index_free(shard.idx);
    std::printf("DOCSET_RANGES_CHECK_OK {\"sets\": %d, \"probe\": %d, \"ids\": %llu, \"hook_calls\": %d, \"lists\": %d}\n", g_sets, g_probe, (unsigned long long)g_ids, g_hook_calls,
                int(lists.size()));
    return 0;
}
