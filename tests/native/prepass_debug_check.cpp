// TEST INFRASTRUCTURE — the vq_debug_*_lists entry points (capi_debug.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own
// (run by tests/test_prepass_debug_cpu.py): built with g++ -fsanitize=address,undefined from the library's host sources and the stubbed device
// layer (hip_stub*.cpp).  With VQ_STUB_NOOP_LAUNCH=1, which this program sets, the launchers return without doing anything and "device" memory is
// zeroed host memory: every driver runs to its end over empty results, so the job tables, the drivers' host side and the copy of every list with
// its 8 trailing entries are walked; then the arguments the functions must refuse (-2) and a failing launch (-1).  Prints PREPASS_DEBUG_CHECK_OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/veloci_amd.h"

extern "C" void vq_stub_fail_launches_after(long k);

#define CHECK(x)                                                                                                    \
    do {                                                                                                            \
        if (!(x)) {                                                                                                 \
            std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, vq_last_error());               \
            std::exit(1);                                                                                           \
        }                                                                                                           \
    } while (0)

int main() {
    setenv("VQ_STUB_NOOP_LAUNCH", "1", 1);
    const uint32_t n_docs = 64, n_tokens = 70;
    // token t: the docs t % 7, t % 7 + 7, ...
    std::vector<uint64_t> off(1, 0);
    std::vector<uint32_t> docs, scores;
    for (uint32_t t = 0; t < n_tokens; ++t) {
        for (uint32_t d = t % 7; d < n_docs; d += 7) {
            docs.push_back(d);
            scores.push_back(1 + t);
        }
        off.push_back(docs.size());
    }
    std::vector<uint64_t> one(n_tokens + 1);
    std::vector<uint32_t> ident(n_tokens);
    for (uint32_t i = 0; i <= n_tokens; ++i) one[i] = i;
    for (uint32_t i = 0; i < n_tokens; ++i) ident[i] = i % n_docs;
    std::vector<uint32_t> boost_bits(n_tokens, 0x3F800000u);
    std::vector<uint8_t> present(n_tokens, 1);
    vq_index_builder* b = vq_index_builder_new(n_docs, 0, n_docs);
    CHECK(b);
    CHECK(vq_index_add_token_to_anchor_score(b, "f.textindex.to_anchor_id_score", n_tokens, off.data(), docs.data(), scores.data(), nullptr) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "f[].textindex.tokens_to_text_id", 0, n_tokens, off.data(), docs.data()) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "f[].textindex.text_id_to_anchor", 3, n_tokens, one.data(), ident.data()) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "f[].textindex.value_id_to_parent", 0, n_tokens, off.data(), docs.data()) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "g[].value_id_to_anchor", 2, n_tokens, one.data(), ident.data()) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "g[].parent_to_value_id", 0, n_tokens, one.data(), ident.data()) == VQ_OK);  // (no image the drivers read)
    CHECK(vq_index_add_boost(b, "g[].boost_valid_to_value", 1, n_tokens, present.data(), boost_bits.data()) == VQ_OK);
    vq_index* idx = nullptr;
    CHECK(vq_index_build(b, 0, &idx) == VQ_OK && idx);
    vq_index_builder_free(b);
    CHECK(vq_profile_enable(idx, 1) == VQ_OK);

    const uint32_t n_jobs = 3;
    const char* post[n_jobs] = {"f.textindex.to_anchor_id_score", "f.textindex.to_anchor_id_score", "f.textindex.to_anchor_id_score"};
    const char* t2t[n_jobs] = {"f[].textindex.tokens_to_text_id", "f[].textindex.tokens_to_text_id", "f[].textindex.tokens_to_text_id"};
    const char* t2a[n_jobs] = {"f[].textindex.text_id_to_anchor", "f[].textindex.text_id_to_anchor", "f[].textindex.text_id_to_anchor"};
    const char* par[n_jobs] = {"f[].textindex.value_id_to_parent", "f[].textindex.value_id_to_parent", "f[].textindex.value_id_to_parent"};
    const char* anc[n_jobs] = {"g[].value_id_to_anchor", "g[].value_id_to_anchor", "g[].value_id_to_anchor"};
    const char* bst[n_jobs] = {"g[].boost_valid_to_value", "g[].boost_valid_to_value", "g[].boost_valid_to_value"};
    // jobs of 1, 3 and 60 ids (one level of k_union: a second level would read counts no kernel wrote); the 1:n and locality jobs use the same ids
    std::vector<uint64_t> job_off = {0, 1, 4, 64};
    std::vector<uint32_t> ids(70), ts_bits(70, 0x3F800000u);
    for (uint32_t i = 0; i < 70; ++i) ids[i] = i % n_tokens;
    const uint64_t cap = 4096;
    std::vector<uint32_t> out_docs(cap), out_bits(cap), len(n_jobs), mx(n_jobs), total(n_jobs), flags(n_jobs);
    size_t ok = 0, refused = 0;
    for (int route = 0; route <= 2; ++route) {
        std::fill(out_docs.begin(), out_docs.end(), 7u);
        CHECK(vq_debug_union_lists(idx, post, job_off.data(), ids.data(), ts_bits.data(), n_jobs, route, cap, len.data(), mx.data(), out_docs.data(), out_bits.data()) == 0);
        for (uint32_t j = 0; j < n_jobs; ++j) CHECK(len[j] == 0 && mx[j] == 0);  // (nothing ran: empty lists, largest value 0.0f)
        CHECK(out_docs[3 * 8 - 1] == 0 && out_docs[3 * 8] == 7u);                // 3 x 8 trailing entries copied, nothing beyond
        ++ok;
    }
    CHECK(vq_debug_union_lists(idx, post, job_off.data(), ids.data(), ts_bits.data(), n_jobs, 1, 3 * 8, len.data(), mx.data(), out_docs.data(), out_bits.data()) == 0);
    CHECK(vq_debug_union_lists(idx, post, job_off.data(), ids.data(), ts_bits.data(), n_jobs, 1, 3 * 8 - 1, len.data(), mx.data(), out_docs.data(), out_bits.data()) == -2);
    CHECK(vq_debug_locality_lists(idx, t2t, t2a, job_off.data(), ids.data(), n_jobs, cap, len.data(), out_docs.data(), out_bits.data()) == 0);
    CHECK(vq_debug_boost1n_lists(idx, par, anc, bst, job_off.data(), ids.data(), n_jobs, cap, len.data(), total.data(), flags.data(), out_docs.data(), out_bits.data()) == 0);
    CHECK(flags[0] == 1u && total[2] == 0);  // (ascending, not several: what an empty list is)
    std::vector<uint64_t> an_off = {0, 2, 2, 5};
    std::vector<uint32_t> anchors = {0, 63, 1, 2, 40};
    std::vector<uint64_t> counts(2 * anchors.size() + 1, 9);
    CHECK(vq_debug_range_hits(idx, post, job_off.data(), ids.data(), an_off.data(), anchors.data(), n_jobs, counts.data()) == 0);
    CHECK(counts[0] == 0 && counts[9] == 0 && counts[10] == 9);
    ok += 4;

    // what the functions refuse
    const char* unknown[n_jobs] = {"f.textindex.to_anchor_id_score", "nope", "f.textindex.to_anchor_id_score"};
    const char* no_image[n_jobs] = {"g[].parent_to_value_id", "g[].parent_to_value_id", "g[].parent_to_value_id"};
    std::vector<uint64_t> empty_job = {0, 1, 1, 64}, not_csr = {0, 4, 1, 64}, not_zero = {1, 1, 4, 64};
    std::vector<uint32_t> big_ids = ids;
    big_ids[2] = n_tokens;
    std::vector<uint32_t> flat = {5, 5, 1, 2, 40};
#define REFUSED(call)     \
    do {                  \
        CHECK((call) == -2); \
        ++refused;        \
    } while (0)
    REFUSED(vq_debug_union_lists(nullptr, post, job_off.data(), ids.data(), ts_bits.data(), n_jobs, 1, cap, len.data(), mx.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_union_lists(idx, unknown, job_off.data(), ids.data(), ts_bits.data(), n_jobs, 1, cap, len.data(), mx.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_union_lists(idx, post, job_off.data(), ids.data(), ts_bits.data(), n_jobs, 3, cap, len.data(), mx.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_union_lists(idx, post, job_off.data(), ids.data(), ts_bits.data(), 0, 1, cap, len.data(), mx.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_union_lists(idx, post, empty_job.data(), ids.data(), ts_bits.data(), n_jobs, 1, cap, len.data(), mx.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_union_lists(idx, post, not_csr.data(), ids.data(), ts_bits.data(), n_jobs, 1, cap, len.data(), mx.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_union_lists(idx, post, not_zero.data(), ids.data(), ts_bits.data(), n_jobs, 1, cap, len.data(), mx.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_union_lists(idx, post, job_off.data(), big_ids.data(), ts_bits.data(), n_jobs, 1, cap, len.data(), mx.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_union_lists(idx, post, job_off.data(), ids.data(), ts_bits.data(), n_jobs, 1, cap, nullptr, mx.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_locality_lists(idx, t2a, t2a, job_off.data(), ids.data(), n_jobs, cap, len.data(), out_docs.data(), out_bits.data()));  // (no CSR image of that table)
    REFUSED(vq_debug_locality_lists(idx, t2t, t2t, job_off.data(), ids.data(), n_jobs, cap, len.data(), out_docs.data(), out_bits.data()));  // (no row table)
    REFUSED(vq_debug_locality_lists(idx, t2t, unknown, job_off.data(), ids.data(), n_jobs, cap, len.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_boost1n_lists(idx, no_image, anc, bst, job_off.data(), ids.data(), n_jobs, cap, len.data(), total.data(), flags.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_boost1n_lists(idx, par, anc, anc, job_off.data(), ids.data(), n_jobs, cap, len.data(), total.data(), flags.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_boost1n_lists(idx, par, anc, bst, job_off.data(), ids.data(), n_jobs, 3 * 8 - 1, len.data(), total.data(), flags.data(), out_docs.data(), out_bits.data()));
    REFUSED(vq_debug_range_hits(idx, post, job_off.data(), ids.data(), an_off.data(), flat.data(), n_jobs, counts.data()));       // anchors that do not ascend
    REFUSED(vq_debug_range_hits(idx, post, job_off.data(), big_ids.data(), an_off.data(), anchors.data(), n_jobs, counts.data()));
    REFUSED(vq_debug_range_hits(idx, unknown, job_off.data(), ids.data(), an_off.data(), anchors.data(), n_jobs, counts.data()));

    // a launch that fails: -1, and the index stays usable
    vq_stub_fail_launches_after(0);
    CHECK(vq_debug_union_lists(idx, post, job_off.data(), ids.data(), ts_bits.data(), n_jobs, 1, cap, len.data(), mx.data(), out_docs.data(), out_bits.data()) == -1);
    vq_stub_fail_launches_after(1);
    CHECK(vq_debug_locality_lists(idx, t2t, t2a, job_off.data(), ids.data(), n_jobs, cap, len.data(), out_docs.data(), out_bits.data()) == -1);
    vq_stub_fail_launches_after(-1);
    CHECK(vq_debug_boost1n_lists(idx, par, anc, bst, job_off.data(), ids.data(), n_jobs, cap, len.data(), total.data(), flags.data(), out_docs.data(), out_bits.data()) == 0);
    const char* prof = vq_profile_json(idx, 1);
    CHECK(std::strstr(prof, "k_union<write>") && std::strstr(prof, "k_union_dense_write") && std::strstr(prof, "k_locality") && std::strstr(prof, "k_boost1n") &&
          std::strstr(prof, "k_range_hits"));
    vq_index_free(idx);
    std::printf("PREPASS_DEBUG_CHECK_OK {\"ok\": %zu, \"refused\": %zu}\n", ok, refused);
    return 0;
}
