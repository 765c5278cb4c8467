// TEST INFRASTRUCTURE — who keeps a request alive (capi_internal.hpp: vq_request shares its request with every batch a caller holds), under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (run by tests/test_request_lifetime_cpu.py): built with g++
// -fsanitize=address,undefined from the library's host sources and the stubbed device layer (hip_stub*.cpp).  With VQ_STUB_NOOP_LAUNCH=1, which
// this program sets, the launchers do nothing and "device" memory is zeroed host memory: steps and partial batches run to their end over empty
// rankings, which walks every place that reads a batch's requests after the call that took them — the further pages of a deep request in
// vq_shard_step_end, the merge of a partial batch.  Each scenario runs twice: with the handles freed as soon as the call that took them has
// returned (and their memory reused by other requests), and, the control, with the handles freed at the very end.  Statuses and counts of both
// must agree; the sanitizers must stay silent.  Prints REQUEST_LIFETIME_CHECK_OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/veloci_amd.h"

#define CHECK(x)                                                                                      \
    do {                                                                                              \
        if (!(x)) {                                                                                   \
            std::fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, vq_last_error()); \
            std::exit(1);                                                                             \
        }                                                                                             \
    } while (0)

static const uint32_t kAnchors = 200003;

static vq_index* build() {
    vq_index_builder* b = vq_index_builder_new(kAnchors, 0, kAnchors);
    CHECK(b);
    const char* terms = "alphabetagamma";
    const uint64_t toff[4] = {0, 5, 9, 14}, off[4] = {0, 3, 5, 9};
    const uint32_t anchors[9] = {1, 70500, 149000, 2, 100000, 1, 2, 70500, 200002}, scores[9] = {10, 10, 10, 10, 10, 10, 10, 10, 10};
    CHECK(vq_index_add_fst(b, "body.textindex", 3, reinterpret_cast<const uint8_t*>(terms), toff) == VQ_OK);
    CHECK(vq_index_add_token_to_anchor_score(b, "body.textindex.to_anchor_id_score", 3, off, anchors, scores, nullptr) == VQ_OK);
    CHECK(vq_index_add_key_value_store(b, "body.textindex.text_id_to_anchor", 0, 3, off, anchors) == VQ_OK);
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

static const std::string kLeaves =
    "{\"search\":{\"path\":\"body\",\"terms\":[\"alpha\"]}},{\"search\":{\"path\":\"body\",\"terms\":[\"beta\"]}},{\"search\":{\"path\":\"body\",\"terms\":[\"gamma\"]}}";
static const std::string kAnd3 = "{\"search_req\":{\"and\":{\"queries\":[" + kLeaves + "]}}}";
static const std::string kOr3 = "{\"search_req\":{\"or\":{\"queries\":[" + kLeaves + "]}},\"top\":7}";
static const std::string kDeep = "{\"search_req\":{\"or\":{\"queries\":[" + kLeaves + "]}},\"top\":10,\"skip\":1100}";  // top + skip > 1024: pages on after its scan

// a plain request, a deep one, a plain one
static std::vector<vq_request*> three() { return {parse(kAnd3), parse(kDeep), parse(kOr3)}; }
static void free_all(std::vector<vq_request*>& reqs) {
    for (vq_request* r : reqs) vq_request_free(r);
    reqs.clear();
}
// requests that take the memory freed handles left behind, with other contents
static void churn() {
    std::vector<vq_request*> other;
    for (int i = 0; i < 24; ++i) other.push_back(parse(i % 2 ? "{\"search_req\":{\"search\":{\"path\":\"nowhere\",\"terms\":[\"zeta\"]}},\"top\":3,\"skip\":5000}" : kAnd3));
    free_all(other);
}

static const size_t kStride = 16;
static size_t g_steps = 0, g_partials = 0, g_freed_early = 0;
static void record_flat(std::string& log, const char* what, size_t n, const std::vector<int>& status, const std::vector<uint64_t>& hits, const std::vector<uint32_t>& counts) {
    log += what;
    for (size_t i = 0; i < n; ++i) log += " " + std::to_string(status[i]) + "/" + std::to_string(hits[i]) + "/" + std::to_string(counts[i]);
    log += "\n";
}
static void end_step(std::string& log, const char* what, vq_shard_step* step, size_t n) {
    std::vector<int> status(n, 77);
    std::vector<uint64_t> hits(n, 77);
    std::vector<uint32_t> counts(n, 77), ids(n * kStride);
    std::vector<float> scores(n * kStride);
    CHECK(vq_shard_step_end(step, kStride, hits.data(), counts.data(), ids.data(), scores.data(), status.data()) == VQ_OK);
    record_flat(log, what, n, status, hits, counts);
    ++g_steps;
}
static const vq_request* const* handles(const std::vector<vq_request*>& v) { return const_cast<const vq_request* const*>(v.data()); }

// 1: two steps in flight, each with a deep request among plain ones
static void steps(const vq_index* idx, bool early, std::string& log) {
    std::vector<vq_request*> a = three(), b = three();
    vq_shard_step *s1 = nullptr, *s2 = nullptr;
    CHECK(vq_shard_step_begin(idx, handles(a), a.size(), &s1) == VQ_OK && s1);
    CHECK(vq_shard_step_begin(idx, handles(b), b.size(), &s2) == VQ_OK && s2);
    if (early) {
        g_freed_early += a.size() + b.size();
        free_all(a);
        free_all(b);
        churn();
    }
    end_step(log, "step 1:", s1, 3);
    end_step(log, "step 2:", s2, 3);
    free_all(a);
    free_all(b);
}

// 2: a partial batch merged after its handles went
static void partials(const vq_index* idx, bool early, std::string& log) {
    std::vector<vq_request*> a = three();
    vq_partial_batch* pb = nullptr;
    CHECK(vq_search_batch_partial(idx, handles(a), a.size(), &pb) == VQ_OK && pb);
    if (early) {
        g_freed_early += a.size();
        free_all(a);
        churn();
    }
    vq_result* out[3] = {nullptr, nullptr, nullptr};
    int status[3] = {77, 77, 77};
    CHECK(vq_merge_partials(idx, pb, nullptr, 1, out, status) == VQ_OK);
    log += "partials:";
    for (size_t i = 0; i < 3; ++i) {
        log += " " + std::to_string(status[i]);
        if (out[i]) log += "/" + std::to_string(vq_result_num_hits(out[i])) + "/" + std::to_string(vq_result_len(out[i])) + "/" + std::to_string(vq_result_is_page(out[i]));
        if (out[i]) vq_result_free(out[i]);
    }
    log += "\n";
    vq_partial_free(pb);
    ++g_partials;
    free_all(a);
}

// 3: a request's doc set replaced while a step made from the request is in flight, the first set's handle freed: the step keeps the request and
// the set it was begun with, the handle goes on with the new set
static void docset_mid_step(const vq_index* idx, const vq_index* other, bool early, std::string& log) {
    const uint32_t ids[4] = {1, 2, 70500, 1}, ids2[2] = {2, 100000};
    vq_docset *first = nullptr, *second = nullptr, *foreign = nullptr;
    CHECK(vq_docset_create(idx, ids, 4, 0, &first) == VQ_OK && vq_docset_create(idx, ids2, 2, 0, &second) == VQ_OK && vq_docset_create(other, ids, 4, 0, &foreign) == VQ_OK);
    std::vector<vq_request*> a = {parse(kAnd3), parse(kAnd3)};
    CHECK(vq_request_set_docset(a[0], first) == VQ_OK);
    vq_shard_step* s = nullptr;
    CHECK(vq_shard_step_begin(idx, handles(a), a.size(), &s) == VQ_OK && s);
    if (early) {
        CHECK(vq_request_set_docset(a[0], second) == VQ_OK);
        vq_docset_free(first);
        first = nullptr;
        ++g_freed_early;
        CHECK(vq_request_set_docset(a[0], foreign) == VQ_OK);  // (and once more: the handle is the copy's only owner now, changed in place)
        churn();
    }
    end_step(log, "doc set:", s, 2);
    if (early) {  // the handle did take the new set: a set of another index is refused at the next use
        vq_shard_step* again = nullptr;
        CHECK(vq_shard_step_begin(idx, handles(a), a.size(), &again) == VQ_OK && again);
        std::string refused;
        end_step(refused, "", again, 2);
        std::fputs(("next use:" + refused).c_str(), stderr);
        CHECK(refused == " " + std::to_string(VQ_ERR_INVALID_ARGUMENT) + "/0/0 0/0/0\n");
    }
    free_all(a);
    if (first) vq_docset_free(first);
    vq_docset_free(second);
    vq_docset_free(foreign);
}

static std::string run(const vq_index* idx, const vq_index* other, bool early) {
    std::string log;
    steps(idx, early, log);
    partials(idx, early, log);
    docset_mid_step(idx, other, early, log);
    return log;
}

int main() {
    setenv("VQ_STUB_NOOP_LAUNCH", "1", 1);
    setenv("VQ_STUB_DICT_SCAN", "1", 1);
    setenv("VQ_HOST_THREADS", "2", 1);
    vq_index* idx = build();
    vq_index* other = build();
    const std::string control = run(idx, other, false);
    const std::string early = run(idx, other, true);
    std::fputs(control.c_str(), stderr);
    if (early != control) {
        std::fprintf(stderr, "FAILED: with the handles freed early\n%sthe control\n%s", early.c_str(), control.c_str());
        return 1;
    }
    // the deep requests came back as ordinary results from the steps (paged to their end) and as page 0 from the merge of the partials
    CHECK(control.find("step 1: 0/0/0 0/0/0 0/0/0\n") == 0 && control.find("partials: 0/0/0/0 0/0/0/1 0/0/0/0\n") != std::string::npos);
    vq_index_free(idx);
    vq_index_free(other);
    std::printf("REQUEST_LIFETIME_CHECK_OK {\"steps\": %zu, \"partial_batches\": %zu, \"handles_freed_early\": %zu}\n", g_steps, g_partials, g_freed_early);
    return 0;
}
