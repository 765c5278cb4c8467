// TEST INFRASTRUCTURE — vq_suggest_batch under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by
// tests/test_suggest_batch_cpu.py): built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device layer
// (hip_stub*.cpp).  It builds a small index through the C ABI and sends batches of good, failing and repeated requests: exact parts (no
// dictionary scan), prefix parts with and without `top` (with VQ_STUB_DICT_SCAN=1, which this program sets, the stubbed launchers answer them on the
// host, in the kernels' formats), every result compared with vq_suggest_json's; everything is freed again.  Prints SUGGEST_BATCH_CHECK_OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static bool same(const vq_suggest_result* a, const vq_suggest_result* b) {
    if (vq_suggest_len(a) != vq_suggest_len(b)) return false;
    for (size_t i = 0; i < vq_suggest_len(a); ++i) {
        const float x = vq_suggest_score(a, i), y = vq_suggest_score(b, i);
        if (std::strcmp(vq_suggest_text(a, i), vq_suggest_text(b, i)) != 0 || std::memcmp(&x, &y, 4) != 0 || vq_suggest_term_id(a, i) != vq_suggest_term_id(b, i)) return false;
    }
    return true;
}

int main() {
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    // 600 sorted terms: "p000" .. "p449" (450 matches of one prefix: the top-n loop cuts), some of other lengths and cases
    std::vector<std::string> terms = {"Foo", "a", "ab", "abc", "abcd", "foo", "foobar"};
    for (int i = 0; i < 450; ++i) {
        char buf[32];
        std::snprintf(buf, sizeof buf, "p%03d%.*s", i, i % 5, "xxxx");
        terms.push_back(buf);
    }
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> toff(1, 0), offsets;
    std::vector<uint32_t> anchors, scores;
    for (size_t i = 0; i < terms.size(); ++i) {
        bytes.insert(bytes.end(), terms[i].begin(), terms[i].end());
        toff.push_back(bytes.size());
        offsets.push_back(i);
        anchors.push_back(uint32_t(i % 16));
        scores.push_back(10);
    }
    offsets.push_back(terms.size());
    vq_index_builder* b = vq_index_builder_new(16, 0, 16);
    CHECK(b);
    CHECK(vq_index_add_fst(b, "f.textindex", uint32_t(terms.size()), bytes.data(), toff.data()) == VQ_OK);
    CHECK(vq_index_add_token_to_anchor_score(b, "f.textindex.to_anchor_id_score", uint32_t(terms.size()), offsets.data(), anchors.data(), scores.data(), nullptr) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "f.textindex.text_id_to_anchor", 0, uint32_t(terms.size()), offsets.data(), anchors.data()) == VQ_OK);
    vq_index* idx = nullptr;
    CHECK(vq_index_build(b, 0, &idx) == VQ_OK && idx);
    vq_index_builder_free(b);

    const std::vector<std::string> reqs = {
        R"({"path":"f","terms":["foo"]})",
        R"({"path":"f","terms":["p"],"starts_with":true,"top":10})",
        R"({"path":"f","terms":["p"],"starts_with":true,"top":10})",
        R"({"path":"f","terms":["p"],"starts_with":true,"top":3,"skip":2})",
        R"({"path":"f","terms":["p"],"starts_with":true})",
        R"({"path":"f","terms":["p)",
        R"({"suggest":[{"path":"f","terms":["a"],"starts_with":true,"top":2},{"path":"f","terms":["Foo"]},{"path":"f","terms":["p1"],"starts_with":true,"top":1848}],"top":7})",
        R"({"path":"nope","terms":["p"],"starts_with":true,"top":10})",
        R"({"path":"f","terms":[],"top":10})",
        R"({"path":"f","terms":["(p"],"is_regex":true})",
        R"({"path":"f","terms":["p"],"starts_with":true,"top":1849})",
        R"({"path":"f","terms":["p00"],"starts_with":true,"top":0})",
        R"({"path":"f","terms":["p"],"starts_with":true,"top":10,"boost":-1.5})",
    };
    std::vector<const char*> text;
    std::vector<size_t> len;
    for (auto& r : reqs) {
        text.push_back(r.c_str());
        len.push_back(r.size());
    }
    size_t good = 0, bad = 0, entries = 0;
    for (int round = 0; round < 2; ++round) {
        std::vector<vq_suggest_result*> out(reqs.size(), nullptr);
        std::vector<int> status(reqs.size(), -1);
        CHECK(vq_suggest_batch(idx, text.data(), len.data(), reqs.size(), out.data(), status.data()) == VQ_OK);
        for (size_t i = 0; i < reqs.size(); ++i) {
            vq_suggest_result* one = nullptr;
            const int rc = vq_suggest_json(idx, text[i], len[i], &one);
            CHECK(rc == status[i]);
            CHECK((rc == VQ_OK) == (out[i] != nullptr) && (rc == VQ_OK) == (one != nullptr));
            if (rc == VQ_OK) {
                CHECK(same(out[i], one));
                entries += vq_suggest_len(one);
                ++good;
                vq_suggest_free(one);
                vq_suggest_free(out[i]);
            } else ++bad;
        }
    }
    CHECK(vq_suggest_batch(idx, nullptr, nullptr, 0, nullptr, nullptr) == VQ_OK);
    CHECK(vq_suggest_batch(nullptr, text.data(), len.data(), 1, nullptr, nullptr) == VQ_ERR_INVALID_ARGUMENT);
    uint64_t topn = 0, records = 0;
    vq_index_suggest_topn_probes(idx, &topn, &records);
    CHECK(topn >= 8 && records > 0);
    vq_index_free(idx);
    std::printf("SUGGEST_BATCH_CHECK_OK {\"good\": %zu, \"failing\": %zu, \"entries\": %zu, \"topn_probes\": %llu, \"records\": %llu}\n", good, bad, entries,
                (unsigned long long)topn, (unsigned long long)records);
    return 0;
}
