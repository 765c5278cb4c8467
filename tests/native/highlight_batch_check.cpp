// TEST INFRASTRUCTURE — vq_highlight_batch under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by
// tests/test_highlight_batch_cpu.py): built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device layer
// (hip_stub*.cpp).  It builds a small tokenized field through the C ABI — a dictionary, tokens_to_text_id and text_id_to_token_ids that agree,
// and a second field whose stores disagree — and sends batches of good, failing and repeated parts: exact and prefix parts with and without
// `top` (with VQ_STUB_DICT_SCAN=1, which this program sets, the stubbed launchers answer the scans and the two text-rank kernels on the host, in
// the kernels' formats), every result compared with vq_highlight_json's; everything is freed again.  Prints HIGHLIGHT_BATCH_CHECK_OK.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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

struct Csr {
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> vals;
    void row(const std::vector<uint32_t>& r) {
        vals.insert(vals.end(), r.begin(), r.end());
        off.push_back(vals.size());
    }
};

// a field of `n_texts` texts "w<i> the w<i+1> [pa<i % 7>]": its dictionary holds the words, the separator and the texts; the two stores either agree
// or, with `drop_text`, text_id_to_token_ids lacks that text's row
static void add_field(vq_index_builder* b, const std::string& field, int n_texts, int drop_text) {
    std::vector<std::string> texts;
    std::map<std::string, uint32_t> ids;
    for (int i = 0; i < n_texts; ++i) {
        std::string t = "w" + std::to_string(i) + " the w" + std::to_string(i + 1);
        if (i % 3 == 0) t += " pa" + std::to_string(i % 7);
        texts.push_back(t);
        ids[t] = 0;
        ids[" "] = 0;
        size_t at = 0;
        while (at < t.size()) {
            size_t sp = t.find(' ', at);
            if (sp == std::string::npos) sp = t.size();
            ids[t.substr(at, sp - at)] = 0;
            at = sp + 1;
        }
    }
    std::vector<std::string> terms;
    for (auto& kv : ids) {  // (std::map: bytewise order, as the dictionary wants it)
        kv.second = uint32_t(terms.size());
        terms.push_back(kv.first);
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
    std::vector<std::vector<uint32_t>> token_rows(terms.size()), text_rows(terms.size());
    for (int i = 0; i < n_texts; ++i) {
        const std::string& t = texts[i];
        const uint32_t text = ids[t];
        size_t at = 0;
        while (at < t.size()) {
            size_t sp = t.find(' ', at);
            if (sp == std::string::npos) sp = t.size();
            text_rows[text].push_back(ids[t.substr(at, sp - at)]);
            if (sp < t.size()) text_rows[text].push_back(ids[" "]);
            at = sp + 1;
        }
        for (uint32_t tok : text_rows[text]) token_rows[tok].push_back(text);
    }
    Csr t2t, tok;
    for (auto& r : token_rows) {
        std::sort(r.begin(), r.end());
        r.erase(std::unique(r.begin(), r.end()), r.end());
        t2t.row(r);
    }
    for (size_t k = 0; k < text_rows.size(); ++k) tok.row(drop_text >= 0 && k == ids[texts[drop_text]] ? std::vector<uint32_t>() : text_rows[k]);
    const std::string p = field + ".textindex";
    CHECK(vq_index_add_fst(b, p.c_str(), uint32_t(terms.size()), bytes.data(), toff.data()) == VQ_OK);
    CHECK(vq_index_add_token_to_anchor_score(b, (p + ".to_anchor_id_score").c_str(), uint32_t(terms.size()), offsets.data(), anchors.data(), scores.data(), nullptr) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, (p + ".text_id_to_anchor").c_str(), 0, uint32_t(terms.size()), offsets.data(), anchors.data()) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, (p + ".tokens_to_text_id").c_str(), 0, uint32_t(terms.size()), t2t.off.data(), t2t.vals.data()) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, (p + ".text_id_to_token_ids").c_str(), 0, uint32_t(terms.size()), tok.off.data(), tok.vals.data()) == VQ_OK);
    CHECK(vq_index_set_column_meta(b, field.c_str(), 0, 1) == VQ_OK);
}

int main() {
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    unsetenv("VQ_NO_HIGHLIGHT_RANK");
    vq_index_builder* b = vq_index_builder_new(16, 0, 16);
    CHECK(b);
    add_field(b, "f", 300, -1);
    add_field(b, "g", 40, 5);
    vq_index* idx = nullptr;
    CHECK(vq_index_build(b, 0, &idx) == VQ_OK && idx);
    vq_index_builder_free(b);

    const std::vector<std::string> reqs = {
        R"({"path":"f","terms":["the"],"snippet":true,"top":10})",
        R"({"path":"f","terms":["the"],"snippet":true,"top":10})",
        R"({"path":"f","terms":["w1"],"starts_with":true,"snippet":true,"top":10})",
        R"({"path":"f","terms":["w1"],"starts_with":true,"snippet":true,"top":3,"skip":2})",
        R"({"path":"f","terms":["pa"],"starts_with":true,"snippet":true,"top":1024})",
        R"({"path":"f","terms":["pa"],"starts_with":true,"snippet":true,"top":1025})",
        R"({"path":"f","terms":["pa"],"starts_with":true,"snippet":true})",
        R"({"path":"f","terms":["the"],"snippet":true,"top":5,"boost":-1.5})",
        R"({"path":"f","terms":["the"],"snippet":true,"top":5,"snippet_info":{"num_words_around_snippet":1,"snippet_start_tag":"<i>","snippet_end_tag":"</i>"}})",
        R"({"path":"f","terms":["the)",
        R"({"path":"f","terms":["the"],"top":5})",
        R"({"path":"nope","terms":["the"],"snippet":true,"top":5})",
        R"({"path":"f","terms":[],"snippet":true,"top":5})",
        R"({"path":"f","terms":["nothere"],"snippet":true,"top":5})",
        R"({"path":"g","terms":["the"],"snippet":true,"top":5})",
        R"({"path":"g","terms":["w30"],"snippet":true,"top":5})",
        R"({"path":"f","terms":["w.*"],"is_regex":true,"snippet":true,"top":7})",
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
        CHECK(vq_highlight_batch(idx, text.data(), len.data(), reqs.size(), out.data(), status.data()) == VQ_OK);
        for (size_t i = 0; i < reqs.size(); ++i) {
            vq_suggest_result* one = nullptr;
            const int rc = vq_highlight_json(idx, text[i], len[i], &one);
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
    CHECK(vq_highlight_batch(idx, nullptr, nullptr, 0, nullptr, nullptr) == VQ_OK);
    CHECK(vq_highlight_batch(nullptr, text.data(), len.data(), 1, nullptr, nullptr) == VQ_ERR_INVALID_ARGUMENT);
    uint64_t device_parts = 0, snippets = 0;
    vq_index_highlight_rank_counts(idx, &device_parts, &snippets);
    vq_index_highlight_rank_counts(idx, nullptr, nullptr);
    CHECK(device_parts >= 12 && snippets > 0);
    // the kernels' debug entry on the stubbed launchers: two rows, a text in both
    const uint64_t off[3] = {0, 3, 5};
    const uint32_t vals[5] = {4, 1, 9, 1, 7}, bits[2] = {0x3F800000u, 0x40000000u};
    uint32_t out_t[4] = {}, out_b[4] = {}, out_n = 0, touched = 0;
    CHECK(vq_debug_text_rank(off, vals, bits, 2, 10, 3, out_t, out_b, &out_n, &touched) == 0);
    CHECK(out_n == 3 && touched == 4 && out_t[0] == 1 && out_t[1] == 7 && out_t[2] == 4 && out_b[0] == 0x40000000u && out_b[2] == 0x3F800000u);
    CHECK(vq_debug_text_rank(off, vals, bits, 2, 9, 3, out_t, out_b, &out_n, &touched) == -2);
    vq_index_free(idx);
    std::printf("HIGHLIGHT_BATCH_CHECK_OK {\"good\": %zu, \"failing\": %zu, \"entries\": %zu, \"device_parts\": %llu, \"snippets_built\": %llu}\n", good, bad, entries,
                (unsigned long long)device_parts, (unsigned long long)snippets);
    return 0;
}
