// TEST INFRASTRUCTURE — the numeric aggregations of a doc set under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by
// tests/test_docset_aggs_cpu.py): built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device layer
// (hip_stub*.cpp; with VQ_STUB_DICT_SCAN=1, which this program sets, hip_stub_docset_aggs.cpp answers the launchers on the host).  It drives
//   a. vq::agg_limbs_to_double, the one rounding of the exact sum, on crafted limb vectors: ties at bit 53 in both directions, a half with a sticky
//      bit, carries through all nine limbs, slots that hold more than 32 bits, pos == neg, results in the float32 denormal range, a borrow through
//      every word;
//   b. vq_docset_aggregate through the C ABI on a small index — a column without presence, one with a presence bitmap, a 1:n column with its
//      value_id_to_anchor table — over a short set, a set with a bitmap and the empty set, with and without edges, several aggregations in one call,
//      against sums computed here (the values are quarter steps: their float64 sums are exact), four threads on one set, every error path;
//   c. two shards as two threads with a generic summing hook: both ranks end with the whole index's answer, bit for bit.
// Everything is freed again.  Prints DOCSET_AGGS_CHECK_OK.
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/veloci_amd.h"

namespace vq {
double agg_limbs_to_double(const uint64_t* pos, const uint64_t* neg);
}

#define CHECK(x)                                                                      \
    do {                                                                              \
        if (!(x)) {                                                                   \
            std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, vq_last_error()); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static int check_rounding() {
    int n = 0;
    auto run = [&](std::vector<uint64_t> pos, std::vector<uint64_t> neg, double want) {
        pos.resize(9, 0);
        neg.resize(9, 0);
        const double got = vq::agg_limbs_to_double(pos.data(), neg.data());
        if (!same_bits(got, want)) {
            std::fprintf(stderr, "FAILED rounding case %d: got %a want %a\n", n, got, want);
            std::exit(1);
        }
        CHECK(same_bits(vq::agg_limbs_to_double(neg.data(), pos.data()), want == 0.0 ? 0.0 : -want));
        ++n;
    };
    const uint64_t b22 = 1ull << 22;  // slot 1 weighs 2^32: b22 there is 2^54
    run({0}, {0}, 0.0);
    run({3}, {}, std::ldexp(3.0, -149));                  // the float32 denormal range
    run({3}, {5}, -std::ldexp(2.0, -149));
    run({1, b22 >> 1}, {}, std::ldexp(1.0, 53 - 149));    // 2^53 + 1: a tie, the even neighbour is below
    run({3, b22 >> 1}, {}, std::ldexp(double((1ull << 53) + 4), -149));  // 2^53 + 3: a tie, the even neighbour is above
    run({2, b22}, {}, std::ldexp(1.0, 54 - 149));         // 2^54 + 2: a tie, down
    run({3, b22}, {}, std::ldexp(double((1ull << 54) + 4), -149));  // half and a sticky bit: up
    run({6, b22}, {}, std::ldexp(double((1ull << 54) + 8), -149));  // a tie, up to the even one
    run({5, b22}, {}, std::ldexp(double((1ull << 54) + 4), -149));  // below half: down
    run({(1ull << 53) - 1}, {}, std::ldexp(double((1ull << 53) - 1), -149));  // 53 bits in one slot: exact
    run({0xFFFFFFFFFFFFFFFFull}, {}, std::ldexp(1.0, 64 - 149));  // 2^64 - 1 rounds up into a new binade
    run({1ull << 32, 0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull}, {},
        std::ldexp(1.0, 288 - 149));  // a carry out of slot 0 runs through all nine limbs: exactly 2^288
    run(std::vector<uint64_t>(9, 0xFFFFFFFFFFFFFFFFull), {}, std::ldexp(1.0, 320 - 149) + std::ldexp(1.0, 288 - 149));  // 2^320 + 2^288 - 2^32 - 1
    run({0, 0, 0, 0, 0, 0, 0, 0, 1}, {1}, std::ldexp(1.0, 256 - 149));  // 2^256 - 1: a borrow through every word, then up
    run({7, 9, 0, 0, 1ull << 40}, {7, 9, 0, 0, 1ull << 40}, 0.0);  // pos == neg
    run({0, 0, 0, 0, 0, 0, 0, 1ull << 31, 0}, {0, 0, 0, 0, 0, 0, 0, 1ull << 31, 1}, -std::ldexp(1.0, 256 - 149));
    // 2^100 + 1 - 2^100 in the value scale: s = 226 and 126 -> limbs 7 and 3
    run({0, 0, 0, 1ull << 23 << 30, 0, 0, 0, 1ull << 23 << 2}, {0, 0, 0, 0, 0, 0, 0, 1ull << 23 << 2}, 1.0);
    return n;
}

static const uint32_t kAnchors = 70003, kLo = 20001, kHi = 50000, kValues = 90001;
using Ids = std::vector<uint32_t>;
static std::vector<float> g_full, g_sparse, g_m;
static std::vector<uint8_t> g_sparse_present, g_m_present;
static std::vector<uint64_t> g_a_off;
static Ids g_a_vals;

static float grid(uint32_t x) { return float(int((x * 2654435761u) >> 19) - 4096) / 4.0f; }  // quarter steps in [-1024, 1024)
static void make_columns() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (uint32_t d = 0; d < kAnchors; ++d) {
        g_full.push_back(grid(d));
        g_sparse.push_back(d % 401u == 7u ? nan : grid(d + 7777u));
        g_sparse_present.push_back(uint8_t((d / 37u) % 3u == 0 || d == kLo || d == kHi - 1));
    }
    g_full[100] = 0.0f, g_full[101] = -0.0f, g_full[30000] = inf, g_full[60000] = 1e-45f;
    g_full[200] = 0x1p100f, g_full[30200] = 1.0f, g_full[60200] = -0x1p100f;  // one on each side of the shard's borders and one inside
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

struct Want {
    uint64_t docs = 0, count = 0, missing = 0, nan = 0;
    double sum = 0.0;  // exact: quarter steps (and the three big ones, whose sum is 1.0, only ever together)
    float min = 0.0f, max = 0.0f;
    bool pos_inf = false;
    std::vector<uint64_t> buckets;
};
static const std::vector<double> kEdges = {-500.25, -3.5, 0.0, 7.75, 250.0};
static void add_value(Want& w, float v, bool with_edges) {
    if (v != v) {
        ++w.nan;
        return;
    }
    if (!w.count || v < w.min) w.min = v + 0.0f;
    if (!w.count || v > w.max) w.max = v + 0.0f;
    ++w.count;
    if (std::isinf(v)) w.pos_inf = true;
    else if (std::fabs(v) < 0x1p99f) w.sum += double(v);
    if (with_edges) {
        size_t b = 0;
        while (b < kEdges.size() && double(v) >= kEdges[b]) ++b;
        ++w.buckets[b];
    }
}
// field 0 full, 1 sparse, 2 m[].v over the whole index
static Want want_of(int field, const Ids& ids, bool with_edges) {
    Want w;
    w.docs = ids.size();
    if (with_edges) w.buckets.assign(kEdges.size() + 1, 0);
    int big = 0;
    if (field == 2) {
        std::vector<uint8_t> in(kAnchors, 0), has(kAnchors, 0);
        for (uint32_t d : ids) in[d] = 1;
        for (uint32_t v = 0; v < kValues; ++v) {
            if (!g_m_present[v] || g_a_off[v] == g_a_off[v + 1] || !in[g_a_vals[g_a_off[v]]]) continue;
            has[g_a_vals[g_a_off[v]]] = 1;
            add_value(w, g_m[v], with_edges);
        }
        for (uint32_t d : ids) w.missing += !has[d];
    } else {
        for (uint32_t d : ids) {
            if (field == 1 && !g_sparse_present[d]) {
                ++w.missing;
                continue;
            }
            const float v = field == 0 ? g_full[d] : g_sparse[d];
            big += std::fabs(v) == 0x1p100f;
            add_value(w, v, with_edges);
        }
    }
    CHECK(big == 0 || big == 2);  // the big pair cancels exactly; the 1.0 between them is an ordinary value
    if (w.pos_inf) w.sum = std::numeric_limits<double>::infinity();
    return w;
}
static void hold(const vq_docset_agg* a, const Want& w) {
    CHECK(a && a->docs == w.docs && a->count == w.count && a->missing == w.missing && a->nan == w.nan);
    CHECK(same_bits(a->sum, w.sum));
    CHECK(std::memcmp(&a->min, &w.min, 4) == 0 && std::memcmp(&a->max, &w.max, 4) == 0);
    CHECK(a->n_buckets == w.buckets.size() && (w.buckets.empty() ? a->buckets == nullptr : std::memcmp(a->buckets, w.buckets.data(), w.buckets.size() * 8) == 0));
}

static const char* const kSpecs =
    "[{\"field\":\"full\"},{\"field\":\"sparse\",\"edges\":[-500.25,-3.5,0.0,7.75,250.0]},{\"field\":\"m[].v\",\"edges\":[-500.25,-3.5,0.0,7.75,250.0]},"
    "{\"field\":\"full\",\"edges\":[-500.25,-3.5,0.0,7.75,250.0]},{\"field\":\"m[].v\"}]";
static const int kSpecField[5] = {0, 1, 2, 0, 2};
static const bool kSpecEdges[5] = {false, true, true, true, false};
static std::atomic<int> g_aggs{0};
static void check_set(const vq_index* idx, const vq_docset* d, const Ids& ids) {
    vq_docset_aggs* out = nullptr;
    CHECK(vq_docset_aggregate(idx, d, kSpecs, std::strlen(kSpecs), &out) == VQ_OK && out && vq_docset_aggs_len(out) == 5 && !vq_docset_aggs_get(out, 5));
    for (size_t i = 0; i < 5; ++i) hold(vq_docset_aggs_get(out, i), want_of(kSpecField[i], ids, kSpecEdges[i]));
    vq_docset_aggs_free(out);
    g_aggs += 5;
}

struct SumHook {  // two ranks as two threads: a barrier-style sum that knows nothing of what it sums
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint64_t> total;
    int waiting = 0, calls = 0;
    uint64_t generation = 0;
    bool fresh = true;  // the next value vector opens a new sum
    // both ranks meet here; the last to arrive runs `then` before anybody goes on
    template <class F>
    void meet(std::unique_lock<std::mutex>& lock, F then) {
        const uint64_t gen = generation;
        if (++waiting == 2) {
            waiting = 0;
            ++generation;
            then();
            cv.notify_all();
        } else {
            cv.wait(lock, [&] { return generation != gen; });
        }
    }
};
static int sum_hook(void* ctx, uint64_t* values, size_t n) {
    SumHook& h = *static_cast<SumHook*>(ctx);
    std::unique_lock<std::mutex> lock(h.mu);
    ++h.calls;
    if (h.fresh) {
        h.total.assign(n, 0);
        h.fresh = false;
    }
    if (h.total.size() != n) return 1;
    for (size_t i = 0; i < n; ++i) h.total[i] += values[i];
    h.meet(lock, [] {});
    std::memcpy(values, h.total.data(), n * 8);
    h.meet(lock, [&] { h.fresh = true; });
    return 0;
}

int main() {
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    setenv("VQ_HOST_THREADS", "2", 1);
    const int rounding_cases = check_rounding();
    make_columns();
    vq_index* whole = build(0, kAnchors);
    Ids dense, few, three = {200, 30200, 60200}, outside;
    for (uint32_t d = 0; d < kAnchors; ++d) {
        if (d % 5 < 2) dense.push_back(d);
        if (d % 997 == 3 || d == 0 || d == 31 || d == kLo - 1 || d == kLo || d == kHi - 1 || d == kHi || d == kAnchors - 1 || (d >= 98 && d < 103) || d % 10000 == 200) few.push_back(d);
        if ((d < kLo || d >= kHi) && d % 1000 == 7) outside.push_back(d);
    }
    const std::vector<Ids> id_lists = {few, dense, three, outside, Ids{}, Ids{30000}, Ids{100, 101}};
    std::vector<vq_docset*> sets;
    for (const Ids& ids : id_lists) {
        vq_docset* d = nullptr;
        CHECK(vq_docset_create(whole, ids.empty() ? nullptr : ids.data(), ids.size(), 0, &d) == VQ_OK && d);
        check_set(whole, d, ids);
        sets.push_back(d);
    }
    {  // the sum of {2^100, 1, -2^100} is 1; a zero comes back as +0.0
        vq_docset_aggs* out = nullptr;
        const char* one = "[{\"field\":\"full\"}]";
        CHECK(vq_docset_aggregate(whole, sets[2], one, std::strlen(one), &out) == VQ_OK && same_bits(vq_docset_aggs_get(out, 0)->sum, 1.0));
        vq_docset_aggs_free(out);
        CHECK(vq_docset_aggregate(whole, sets[6], one, std::strlen(one), &out) == VQ_OK);
        const float zero = 0.0f;
        CHECK(std::memcmp(&vq_docset_aggs_get(out, 0)->min, &zero, 4) == 0 && std::memcmp(&vq_docset_aggs_get(out, 0)->max, &zero, 4) == 0);
        vq_docset_aggs_free(out);
    }
    {  // four threads on one set
        std::vector<std::thread> pool;
        std::vector<int> good(4, 0);
        const Want want = want_of(2, few, true);
        for (int t = 0; t < 4; ++t)
            pool.emplace_back([&, t] {
                for (int k = 0; k < 3; ++k) {
                    vq_docset_aggs* out = nullptr;
                    if (vq_docset_aggregate(whole, sets[0], kSpecs, std::strlen(kSpecs), &out) != VQ_OK || !out) return;
                    const vq_docset_agg* a = vq_docset_aggs_get(out, 2);
                    const bool same = a->count == want.count && a->missing == want.missing && same_bits(a->sum, want.sum) && std::memcmp(a->buckets, want.buckets.data(), 48) == 0;
                    vq_docset_aggs_free(out);
                    if (!same) return;
                }
                good[t] = 1;
            });
        for (auto& t : pool) t.join();
        CHECK(good == std::vector<int>(4, 1));
    }
    // two shards as two threads
    vq_index* shards[2] = {build(0, kLo + 9000), build(kLo + 9000, kAnchors)};
    SumHook hook;
    {  // a shard without the hook declines, naming it
        vq_docset *d = nullptr;
        vq_docset_aggs* out = nullptr;
        CHECK(vq_docset_create(shards[1], few.data(), few.size(), 0, &d) == VQ_OK);
        CHECK(vq_docset_aggregate(shards[1], d, kSpecs, std::strlen(kSpecs), &out) == VQ_ERR_UNSUPPORTED && !out && std::strstr(vq_last_error(), "vq_index_set_allreduce"));
        vq_docset_free(d);
    }
    for (vq_index* s : shards) CHECK(vq_index_set_allreduce(s, sum_hook, &hook) == VQ_OK);
    {
        std::vector<std::thread> pool;
        std::vector<int> good(2, 0);
        for (int rank = 0; rank < 2; ++rank)
            pool.emplace_back([&, rank] {
                for (const Ids& ids : id_lists) {  // both ranks make the same calls in the same order
                    vq_docset* d = nullptr;
                    if (vq_docset_create(shards[rank], ids.empty() ? nullptr : ids.data(), ids.size(), 0, &d) != VQ_OK) return;
                    check_set(shards[rank], d, ids);
                    vq_docset_free(d);
                }
                good[rank] = 1;
            });
        for (auto& t : pool) t.join();
        CHECK(good == std::vector<int>(2, 1));
        CHECK(hook.calls == 2 * 5 * int(id_lists.size() - 1));  // five per call and rank; none for the empty set
    }
    // misuse
    vq_docset_aggs* out = nullptr;
    vq_docset* foreign = nullptr;
    CHECK(vq_docset_create(shards[0], few.data(), few.size(), 0, &foreign) == VQ_OK);
    const char* fine = "[{\"field\":\"full\"}]";
    CHECK(vq_docset_aggregate(whole, foreign, fine, std::strlen(fine), &out) == VQ_ERR_INVALID_ARGUMENT && !out && std::strstr(vq_last_error(), "another index"));
    CHECK(vq_docset_aggregate(nullptr, sets[0], fine, std::strlen(fine), &out) == VQ_ERR_INVALID_ARGUMENT && vq_docset_aggregate(whole, nullptr, fine, std::strlen(fine), &out) == VQ_ERR_INVALID_ARGUMENT);
    CHECK(vq_docset_aggregate(whole, sets[0], nullptr, 0, &out) == VQ_ERR_INVALID_ARGUMENT && vq_docset_aggregate(whole, sets[0], fine, std::strlen(fine), nullptr) == VQ_ERR_INVALID_ARGUMENT);
    for (const char* bad : {"[{\"field\":\"full\"", "{\"field\":\"full\"}", "[{\"field\":\"full\",\"edges\":[\"1\"]}]", "[{\"field\":\"full\",\"edges\":3}]", "[{\"field\":7}]", "[3]"})
        CHECK(vq_docset_aggregate(whole, sets[0], bad, std::strlen(bad), &out) == VQ_ERR_JSON && !out);
    std::string many = "[{\"field\":\"full\",\"edges\":[";
    for (int i = 0; i < 1024; ++i) many += (i ? "," : "") + std::to_string(i);
    many += "]}]";
    for (const char* bad : {"[]", "[{\"edges\":[1]}]", "[{\"field\":\"full\",\"edge\":[1]}]", "[{\"field\":\"full\",\"edges\":[2,1]}]", "[{\"field\":\"full\",\"edges\":[1,1]}]",
                            "[{\"field\":\"body.textindex.token_values\"}]", many.c_str()})
        CHECK(vq_docset_aggregate(whole, sets[0], bad, std::strlen(bad), &out) == VQ_ERR_INVALID_ARGUMENT && !out);
    const char* unknown = "[{\"field\":\"nosuch\"}]";
    CHECK(vq_docset_aggregate(whole, sets[0], unknown, std::strlen(unknown), &out) == VQ_ERR_INDEX_NOT_FOUND && !out &&
          std::strcmp(vq_last_error(), "Did not found path in indices nosuch.boost_valid_to_value") == 0);
    const char* orphan = "[{\"field\":\"orphan[].v\"}]";
    CHECK(vq_docset_aggregate(whole, sets[0], orphan, std::strlen(orphan), &out) == VQ_ERR_INDEX_NOT_FOUND && !out &&
          std::strcmp(vq_last_error(), "Did not found path in indices orphan[].v.value_id_to_anchor") == 0);
    CHECK(vq_docset_aggs_len(nullptr) == 0 && !vq_docset_aggs_get(nullptr, 0));
    vq_docset_aggs_free(nullptr);
    vq_docset_free(foreign);
    for (vq_docset* d : sets) vq_docset_free(d);
    vq_index_free(whole);
    for (vq_index* s : shards) vq_index_free(s);
    std::printf("DOCSET_AGGS_CHECK_OK {\"rounding\": %d, \"aggs\": %d, \"hook_calls\": %d}\n", rounding_cases, g_aggs.load(), hook.calls);
    return 0;
}
