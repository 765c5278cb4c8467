// TEST INFRASTRUCTURE — the facet counts of a doc set under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by
// tests/test_docset_facets_cpu.py): built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device layer
// (hip_stub*.cpp; with VQ_STUB_DICT_SCAN=1, which this program sets, hip_stub_docset_facets.cpp answers the launchers on the host).  It builds a
// small index and a shard of it through the C ABI — a direct store with fewer keys than anchors, a CSR store with a 5 000-value row and a
// histogram longer than the LDS bound, a composed (two-step) store with a value beyond its dictionary — and drives vq_docset_facets: both
// counting modes with VQ_NO_DOCSET_FACET_LDS flipped in-process, device-ranked and host-ranked tops, the sum over the shards through the hook,
// four threads on one set, and every error path; the answers are held against counts and the ranking rule computed here.  Everything is freed
// again.  Prints DOCSET_FACETS_CHECK_OK.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
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
static const uint32_t kCatKeys = 150010, kCatTerms = 7, kTagTerms = 4097, kFewTerms = 3, kFewValues = 5, kLongRow = 100003, kBeyond = 100005;
using Ids = std::vector<uint32_t>;
using Entries = std::vector<std::pair<std::string, uint64_t>>;

struct Field {
    std::string name;
    std::vector<uint64_t> off;  // rows of the anchors [0, keys)
    Ids vals;
    uint32_t keys, terms, num_values;
    const char* prefix;
};
static Field g_fields[3];

static std::string term_of(const Field& f, uint32_t v) {
    if (v >= f.terms) return "";
    char buf[32];
    std::snprintf(buf, sizeof buf, "%s%05u", f.prefix, v);
    return buf;
}
static void make_fields() {
    Field& cat = g_fields[0];
    cat = Field{"cat", {0}, {}, kCatKeys, kCatTerms, kCatTerms, "c"};
    for (uint32_t d = 0; d < kCatKeys; ++d) {
        if (d % 5) cat.vals.push_back(d % kCatTerms);
        cat.off.push_back(cat.vals.size());
    }
    Field& tags = g_fields[1];
    tags = Field{"tags[]", {0}, {}, kAnchors, kTagTerms, kTagTerms, "t"};
    for (uint32_t d = 0; d < kAnchors; ++d) {
        if (d == kLongRow)
            for (uint32_t j = 0; j < 5000; ++j) tags.vals.push_back((j * 3u) % kTagTerms);
        else if (d % 3 == 0) {
            tags.vals.push_back((d * 7u) % kTagTerms);
            tags.vals.push_back((d * 7u) % kTagTerms == 11u ? 11u : (d * 13u) % kTagTerms);  // (some rows hold one value twice)
        }
        tags.off.push_back(tags.vals.size());
    }
    Field& few = g_fields[2];  // the composed rows: what anchor -> value id -> text id gives
    few = Field{"few[]", {0}, {}, kAnchors, kFewTerms, kFewValues, "f"};
    for (uint32_t d = 0; d < kAnchors; ++d) {
        if (d % 4 == 1) few.vals.push_back(d == kBeyond ? 4u : (d / 4u) % 3u);
        few.off.push_back(few.vals.size());
    }
}

static std::vector<uint64_t> counts_of(const Field& f, const Ids& ids, uint32_t lo, uint32_t hi) {
    std::vector<uint64_t> c(f.num_values, 0);
    for (uint32_t d : ids) {
        if (d < lo || d >= hi || d >= f.keys) continue;
        for (uint64_t e = f.off[d]; e < f.off[d + 1]; ++e)
            if (f.vals[e] < f.num_values) ++c[f.vals[e]];
    }
    return c;
}
static Entries ranked(const Field& f, const std::vector<uint64_t>& c, long top) {  // top < 0: null
    Ids order;
    for (uint32_t v = 0; v < c.size(); ++v)
        if (c[v]) order.push_back(v);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return c[x] != c[y] ? c[x] > c[y] : x < y; });
    if (top >= 0 && order.size() > size_t(top)) order.resize(size_t(top));
    Entries out;
    for (uint32_t v : order) out.push_back({term_of(f, v), c[v]});
    return out;
}

static void add_fst(vq_index_builder* b, const std::string& path, const Field& f) {
    std::string bytes;
    std::vector<uint64_t> off{0};
    for (uint32_t v = 0; v < f.terms; ++v) {
        bytes += term_of(f, v);
        off.push_back(bytes.size());
    }
    CHECK(vq_index_add_fst(b, path.c_str(), f.terms, reinterpret_cast<const uint8_t*>(bytes.data()), off.data()) == VQ_OK);
}
// rows [a, b) of a store as one of key_base a
static void add_rows(vq_index_builder* b, const std::string& path, const std::vector<uint64_t>& off, const Ids& vals, uint32_t a, uint32_t e) {
    std::vector<uint64_t> cut(off.begin() + a, off.begin() + e + 1);
    for (auto& x : cut) x -= off[a];
    CHECK(vq_index_add_key_value_store(b, path.c_str(), a, e - a, cut.data(), vals.data() + off[a]) == VQ_OK);
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
    const Field &cat = g_fields[0], &tags = g_fields[1], &few = g_fields[2];
    add_fst(b, "cat.textindex", cat);
    add_rows(b, "cat.textindex.parent_to_value_id", cat.off, cat.vals, std::min(lo, cat.keys), std::min(hi, cat.keys));
    add_fst(b, "tags[].textindex", tags);
    add_rows(b, "tags[].textindex.anchor_to_text_id", tags.off, tags.vals, lo, hi);
    add_fst(b, "few[].textindex", few);
    {  // anchor -> value id (the row's position in few.vals), value id -> text id: composed on first use
        Ids value_ids(few.vals.size());
        std::vector<uint64_t> one(few.vals.size() + 1);
        for (size_t i = 0; i < value_ids.size(); ++i) value_ids[i] = uint32_t(i);
        for (size_t i = 0; i < one.size(); ++i) one[i] = i;
        add_rows(b, "few[].parent_to_value_id", few.off, value_ids, lo, hi);
        CHECK(vq_index_add_key_value_store(b, "few[].textindex.parent_to_value_id", 0, uint32_t(few.vals.size()), one.data(), few.vals.data()) == VQ_OK);
    }
    vq_index* idx = nullptr;
    CHECK(vq_index_build(b, 0, &idx) == VQ_OK && idx);
    vq_index_builder_free(b);
    return idx;
}

struct Ask {
    int field;
    long top;  // < 0: null
};
static std::string json_of(const std::vector<Ask>& asks) {
    std::string s = "[";
    for (size_t i = 0; i < asks.size(); ++i) {
        s += std::string(i ? "," : "") + "{\"field\":\"" + g_fields[asks[i].field].name + "\",\"top\":" + (asks[i].top < 0 ? std::string("null") : std::to_string(asks[i].top)) + "}";
    }
    return s + "]";
}

// what the shard's hook expects to be handed and answers: set by the caller before every call
static std::vector<uint64_t> g_local, g_whole;
static int g_hook_calls = 0, g_hook_bad = 0;
static int hook(void*, uint64_t* values, size_t n) {
    ++g_hook_calls;
    if (n != g_local.size() || !std::equal(g_local.begin(), g_local.end(), values)) {
        ++g_hook_bad;
        return 1;
    }
    std::copy(g_whole.begin(), g_whole.end(), values);
    return 0;
}

struct Side {
    vq_index* idx;
    uint32_t lo, hi;
};
static int g_calls = 0, g_entries = 0;

static void holds(const Side& s, const vq_docset* d, const Ids& ids, const std::vector<Ask>& asks) {
    g_local.clear();
    g_whole.clear();
    for (const Ask& a : asks) {
        const auto l = counts_of(g_fields[a.field], ids, s.lo, s.hi), w = counts_of(g_fields[a.field], ids, 0, kAnchors);
        g_local.insert(g_local.end(), l.begin(), l.end());
        g_whole.insert(g_whole.end(), w.begin(), w.end());
    }
    const std::string text = json_of(asks);
    for (int forced = 0; forced < 2; ++forced) {
        if (forced) setenv("VQ_NO_DOCSET_FACET_LDS", "1", 1);
        vq_result* r = nullptr;
        CHECK(vq_docset_facets(s.idx, d, text.data(), text.size(), &r) == VQ_OK && r);
        if (forced) unsetenv("VQ_NO_DOCSET_FACET_LDS");
        CHECK(vq_result_num_hits(r) == ids.size() && vq_result_len(r) == 0 && vq_result_num_facets(r) == asks.size());
        for (size_t f = 0; f < asks.size(); ++f) {
            const Field& fd = g_fields[asks[f].field];
            const Entries want = ranked(fd, counts_of(fd, ids, 0, kAnchors), asks[f].top);
            CHECK(fd.name == vq_result_facet_field(r, f) && vq_result_facet_len(r, f) == want.size());
            for (size_t i = 0; i < want.size(); ++i) CHECK(want[i].first == vq_result_facet_value(r, f, i) && want[i].second == vq_result_facet_count(r, f, i));
            g_entries += int(want.size());
        }
        CHECK(std::strstr(vq_result_to_json(r), asks.empty() ? "\"num_hits\"" : "\"facets\""));
        vq_result_free(r);
        ++g_calls;
    }
}

int main() {
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    setenv("VQ_HOST_THREADS", "2", 1);
    unsetenv("VQ_NO_DOCSET_FACET_LDS");
    make_fields();
    const Side whole{build(0, kAnchors), 0, kAnchors}, shard{build(kLo, kHi), kLo, kHi};
    const std::vector<Ask> all_null = {{0, -1}, {1, -1}, {2, -1}}, tops = {{1, 10}, {1, 1024}, {1, 1025}, {0, 0}, {0, 1}, {2, 2}, {1, 10}};
    vq_result* r = nullptr;
    Ids every, thirds, few = {0, 31, 70001, kLongRow, kLongRow + 1, kBeyond, 149999, kAnchors - 1}, outside = {0, 3, 9, 70000, 150000, 150003};
    for (uint32_t d = 0; d < kAnchors; ++d) {
        every.push_back(d);
        if (d % 3 == 0 || d == kBeyond) thirds.push_back(d);
    }
    {  // a shard without the hook declines, naming it; an empty facet list has nothing to sum
        vq_docset* d = nullptr;
        CHECK(vq_docset_create(shard.idx, few.data(), few.size(), 0, &d) == VQ_OK);
        const std::string text = json_of({{0, 3}});
        CHECK(vq_docset_facets(shard.idx, d, text.data(), text.size(), &r) == VQ_ERR_UNSUPPORTED && !r && std::strstr(vq_last_error(), "vq_index_set_allreduce"));
        CHECK(vq_docset_facets(shard.idx, d, "[]", 2, &r) == VQ_OK && r && vq_result_num_facets(r) == 0 && vq_result_num_hits(r) == few.size());
        vq_result_free(r);
        vq_docset_free(d);
    }
    CHECK(vq_index_set_allreduce(shard.idx, hook, nullptr) == VQ_OK);
    for (const Side& s : {whole, shard}) {
        const int hooks_before = g_hook_calls, calls_before = g_calls;
        for (const Ids* ids : {&few, &thirds, &every, &outside}) {
            vq_docset* d = nullptr;
            CHECK(vq_docset_create(s.idx, ids->data(), ids->size(), 0, &d) == VQ_OK && d);
            holds(s, d, *ids, all_null);
            holds(s, d, *ids, tops);
            holds(s, d, *ids, {});
            if (ids == &thirds) {  // four threads on one set (the whole index: the hook of the shard is one conversation)
                const std::string text = json_of(tops);
                if (!s.lo) {
                    std::vector<std::thread> pool;
                    std::vector<int> ok(4, 0);
                    for (int t = 0; t < 4; ++t)
                        pool.emplace_back([&, t] {
                            for (int k = 0; k < 3; ++k) {
                                vq_result* q = nullptr;
                                if (vq_docset_facets(s.idx, d, text.data(), text.size(), &q) != VQ_OK || !q) return;
                                const Entries want = ranked(g_fields[1], counts_of(g_fields[1], thirds, 0, kAnchors), 1024);
                                bool same = vq_result_facet_len(q, 1) == want.size();
                                for (size_t i = 0; same && i < want.size(); ++i) same = want[i].first == vq_result_facet_value(q, 1, i) && want[i].second == vq_result_facet_count(q, 1, i);
                                vq_result_free(q);
                                if (!same) return;
                            }
                            ok[t] = 1;
                        });
                    for (auto& t : pool) t.join();
                    CHECK(ok == std::vector<int>(4, 1));
                }
            }
            vq_docset_free(d);
        }
        vq_docset* empty = nullptr;
        CHECK(vq_docset_create(s.idx, nullptr, 0, 0, &empty) == VQ_OK);
        const int before = g_hook_calls;
        holds(s, empty, Ids{}, all_null);  // nothing is launched, nothing summed: every field with an empty list
        CHECK(g_hook_calls == before);
        // misuse
        vq_docset* d = nullptr;
        CHECK(vq_docset_create(s.idx, few.data(), few.size(), 0, &d) == VQ_OK);
        const Side& other = s.lo ? whole : shard;
        const std::string ok_text = json_of({{0, 3}});
        CHECK(vq_docset_facets(other.idx, d, ok_text.data(), ok_text.size(), &r) == VQ_ERR_INVALID_ARGUMENT && !r && std::strstr(vq_last_error(), "another index"));
        CHECK(vq_docset_facets(nullptr, d, ok_text.data(), ok_text.size(), &r) == VQ_ERR_INVALID_ARGUMENT && vq_docset_facets(s.idx, nullptr, ok_text.data(), ok_text.size(), &r) == VQ_ERR_INVALID_ARGUMENT);
        CHECK(vq_docset_facets(s.idx, d, nullptr, 0, &r) == VQ_ERR_INVALID_ARGUMENT && vq_docset_facets(s.idx, d, ok_text.data(), ok_text.size(), nullptr) == VQ_ERR_INVALID_ARGUMENT);
        for (const char* bad : {"[{\"field\": \"cat\"", "{\"field\": \"cat\"}", "[{\"top\": 3}]", "[7]", "[{\"field\": \"cat\", \"top\": -1}]"})
            CHECK(vq_docset_facets(s.idx, d, bad, std::strlen(bad), &r) == VQ_ERR_JSON && !r);
        const char* unknown = "[{\"field\": \"nosuch\"}]";
        CHECK(vq_docset_facets(s.idx, d, unknown, std::strlen(unknown), &r) == VQ_ERR_INDEX_NOT_FOUND && !r && std::strstr(vq_last_error(), "nosuch.textindex.parent_to_value_id"));
        CHECK(vq_docset_facets(s.idx, d, "null", 4, &r) == VQ_OK && r && vq_result_num_facets(r) == 0);
        vq_result_free(r);
        r = nullptr;
        vq_docset_free(d);
        vq_docset_free(empty);
        if (s.lo) CHECK(g_hook_calls - hooks_before == 2 * 2 * 4 && g_calls - calls_before == 2 * (3 * 4 + 1));  // the hook: once per call with facets on a set that is not empty
        else CHECK(g_hook_calls == hooks_before);                                                                     // an unsharded index never calls it
    }
    CHECK(g_hook_bad == 0);
    vq_index_free(whole.idx);
    vq_index_free(shard.idx);
    std::printf("DOCSET_FACETS_CHECK_OK {\"calls\": %d, \"entries\": %d, \"hook_calls\": %d}\n", g_calls, g_entries, g_hook_calls);
    return 0;
}
