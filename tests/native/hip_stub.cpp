// TEST INFRASTRUCTURE — the device layer stubbed for the CPU sanitizer build (`make -C veloci_amd/csrc asan`, tests/test_host_asan.py): the HIP
// runtime calls the host side makes are mapped to host memory, every kernel launcher throws (one exception, opt-in: with VQ_STUB_DICT_SCAN=1
// exact / prefix dictionary probes are answered by a plain loop, see launch_dict_scan below).  What this build can run is everything in front of
// the first launch: index staging (index.cpp), request parsing, query compilation (compile.cpp, term_lookup.cpp), the C ABI's argument handling — under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Never linked into the product library.
// With VQ_STUB_LAUNCH_LOG=<file> every launcher appends one JSON line to that file (tests/test_launch_plan_cpu.py): its name and scalar arguments; a
// scan launcher also the span_base / qmap tables it was handed ("device" memory is host memory here) and which of its output pointers are set.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>

#include "../../veloci_amd/csrc/engine.hpp"

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
    *p = std::calloc(n ? n : 1, 1);  // zeroed: what a launch that did nothing "wrote" reads the same in every run (the recorded launch plan depends on it)
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) {
    std::free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { return hipMalloc(p, n); }
hipError_t hipHostFree(void* p) { return hipFree(p); }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
    std::memcpy(d, s, n);
    return hipSuccess;
}
static std::atomic<long> g_async_calls{0};  // hipMemcpyAsync + hipMemsetAsync calls so far (tests/native/staging_check.cpp: an empty section issues none)
long vq_stub_async_calls() { return g_async_calls.load(); }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
    ++g_async_calls;
    std::memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) {
    std::memset(d, v, n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) {
    ++g_async_calls;
    std::memset(d, v, n);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) {
    *s = reinterpret_cast<hipStream_t>(std::malloc(8));
    return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) {
    *s = reinterpret_cast<hipStream_t>(std::malloc(8));
    return hipSuccess;
}
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) {
    *lo = 0;
    *hi = -1;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    std::free(s);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) {
    *e = reinterpret_cast<hipEvent_t>(std::malloc(8));
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned int) { return hipEventCreate(e); }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) {
    std::free(e);
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
    *ms = 0.0f;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stubbed HIP runtime"; }
hipError_t hipGetDeviceCount(int* n) {
    *n = 1;
    return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) {
    *d = 0;
    return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int) {
    *v = 256;
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
void vq_stub_fail_launches_after(long k);
}

namespace vq {
// VQ_STUB_NOOP_LAUNCH=1 (tools/host_step_profile.py only): launches do nothing instead of throwing, so that the host side of a whole step
// (compile, pack, launch calls, result assembly — over garbage "results") can be timed on a machine without a GPU
// vq_stub_fail_launches_after(k) (tests/native/gloo_step_driver.py): the k+1-th launch from now and every later one fail — a device error in the
// middle of a step, on one rank only; k < 0 switches it off again
static std::atomic<long> g_fail_after{-1};
void stub_set_fail_after(long k) { g_fail_after.store(k); }
static void no_device(const char* what) {
    static const bool noop = std::getenv("VQ_STUB_NOOP_LAUNCH") != nullptr;
    if (g_fail_after.load() >= 0 && g_fail_after.fetch_sub(1) <= 0) {
        g_fail_after.store(0);
        throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: injected failure of ") + what);
    }
    if (noop) return;
    throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: ") + what);
}
static void log_launch(const char* name, std::initializer_list<long long> scalars, const uint32_t* span_base = nullptr, const uint32_t* qmap = nullptr, uint32_t nq = 0) {
    static const char* path = std::getenv("VQ_STUB_LAUNCH_LOG");
    if (!path) return;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    std::FILE* f = std::fopen(path, "a");
    if (!f) return;
    std::fprintf(f, "{\"launch\":\"%s\",\"args\":[", name);
    const char* sep = "";
    for (long long v : scalars) std::fprintf(f, "%s%lld", sep, v), sep = ",";
    std::fprintf(f, "]");
    if (span_base) {
        std::fprintf(f, ",\"span_base\":[");
        for (uint32_t i = 0; i <= nq; ++i) std::fprintf(f, "%s%u", i ? "," : "", span_base[i]);
        std::fprintf(f, "],\"qmap\":[");
        for (uint32_t i = 0; i < nq; ++i) std::fprintf(f, "%s%u", i ? "," : "", qmap[i]);
        std::fprintf(f, "]");
    }
    std::fprintf(f, "}\n");
    std::fclose(f);
}
size_t tile_scan_lds_bytes(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, bool, uint32_t) { return 0; }
size_t scan_simple_lds_bytes(uint32_t, uint32_t, uint32_t, bool) { return 0; }
size_t scan_wide_lds_bytes(uint32_t, uint32_t, uint32_t) { return 0; }
size_t scan_probe_lds_bytes(uint32_t, uint32_t, uint32_t, uint32_t) { return 0; }
uint32_t debug_probe_occupancy(uint32_t, size_t) { return 0; }
int debug_facet_select(const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t*, uint32_t*) { return -1; }
uint32_t debug_div100_mismatches() {
    no_device("debug_div100_mismatches");
    return 0;
}
// ---- the scan launchers
void launch_tile_scan(hipStream_t, uint32_t total_spans, size_t lds_bytes, const uint8_t*, const uint32_t*, const uint32_t* span_base, const uint32_t* qmap, uint32_t nq,
                      uint32_t stack_depth, uint32_t cand_cap, uint32_t desc_cap, unsigned long long*, unsigned long long*, uint32_t* hist, bool queue, uint32_t ml, bool facet_cache) {
    log_launch("k_tile_scan", {total_spans, (long long)lds_bytes, nq, stack_depth, cand_cap, desc_cap, hist != nullptr, queue, ml, facet_cache}, span_base, qmap, nq);
    no_device("k_tile_scan");
}
void launch_scan_leaf_f32(hipStream_t, uint32_t total_spans, const uint8_t*, const uint32_t*, const uint32_t* span_base, const uint32_t* qmap, uint32_t nq, uint32_t cand_cap,
                          unsigned long long*, unsigned long long*, uint32_t* hist) {
    log_launch("k_scan_leaf_f32", {total_spans, nq, cand_cap, hist != nullptr}, span_base, qmap, nq);
    no_device("k_scan_leaf_f32");
}
void launch_scan_simple(hipStream_t, bool wide, uint32_t n_scatter, uint32_t total_spans, const uint8_t*, const uint32_t*, const uint32_t* span_base, const uint32_t* qmap, uint32_t nq,
                        uint32_t cand_cap, unsigned long long*, unsigned long long*, uint32_t* hist, bool facet_cache) {
    log_launch("k_scan_simple", {wide, n_scatter, total_spans, nq, cand_cap, hist != nullptr, facet_cache}, span_base, qmap, nq);
    no_device("k_scan_simple");
}
void launch_scan_wide(hipStream_t, uint32_t max_leaves, uint32_t max_scatter, uint32_t total_spans, const uint8_t*, const uint32_t*, const uint32_t* span_base, const uint32_t* qmap,
                      uint32_t nq, uint32_t cand_cap, unsigned long long*, unsigned long long*) {
    log_launch("k_scan_wide", {max_leaves, max_scatter, total_spans, nq, cand_cap}, span_base, qmap, nq);
    no_device("k_scan_wide");
}
void launch_scan_probe_shape(hipStream_t, uint32_t shape, uint32_t na_seen, uint32_t arr_slot, uint32_t total_spans, const uint8_t*, const uint32_t*, const uint32_t* span_base,
                             const uint32_t* qmap, uint32_t nq, uint32_t cand_cap, unsigned long long*, unsigned long long*) {
    log_launch("k_scan_probe", {shape, na_seen, arr_slot, total_spans, nq, cand_cap}, span_base, qmap, nq);
    no_device("k_scan_probe");
}
void launch_scan_union(hipStream_t, bool with_or, uint32_t total_spans, const uint8_t*, const uint32_t*, const uint32_t* span_base, const uint32_t* qmap, uint32_t nq, uint32_t cand_cap,
                       unsigned long long*, unsigned long long*) {
    log_launch("k_scan_union", {with_or, total_spans, nq, cand_cap}, span_base, qmap, nq);
    no_device("k_scan_union");
}
// ---- merge and pre-pass launchers
void launch_merge_spans(hipStream_t, uint32_t nq, const uint8_t*, const uint32_t*, const unsigned long long*, unsigned long long*) {
    log_launch("k_merge_spans", {nq});
    no_device("k_merge_spans");
}
void launch_finalize(hipStream_t, uint32_t nq, const uint8_t*, const uint32_t*, const uint8_t*, uint32_t num_shards, size_t, const PartialLayout&, uint32_t*, float*, uint32_t*,
                     unsigned long long*) {
    log_launch("k_finalize", {nq, num_shards});
    no_device("k_finalize");
}
void launch_facet_select(hipStream_t, uint32_t n_jobs, const FacetJob*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*) {
    log_launch("k_facet_select", {n_jobs});
    no_device("k_facet_select");
}
void launch_range_hits(hipStream_t, uint32_t n_blocks, uint32_t n_jobs, const UList*, const RangeJobD*, const uint32_t*, unsigned long long*) {
    log_launch("k_range_hits", {n_blocks, n_jobs});
    no_device("k_range_hits");
}
void launch_union(hipStream_t, bool write, uint32_t total_spans, const UList*, const UTask*, const uint32_t*, uint32_t*, const uint64_t*, uint32_t*, float*, uint32_t*) {
    log_launch("k_union", {write, total_spans});
    no_device("k_union");
}
void launch_union_dense_scatter(hipStream_t, const UDenseList*, uint32_t n_lists, uint64_t total_postings, const UDenseJob*, uint32_t*, uint32_t lo_doc, uint32_t range) {
    log_launch("k_union_dense_scatter", {n_lists, (long long)total_postings, lo_doc, range});
    no_device("k_union_dense_scatter");
}
void launch_union_dense_count(hipStream_t, const UDenseJob*, uint32_t n_jobs, uint32_t n_blocks, const uint32_t*, uint32_t*, uint32_t*, UDenseResult*) {
    log_launch("k_union_dense_count", {n_jobs, n_blocks});
    no_device("k_union_dense_count");
}
void launch_union_dense_write(hipStream_t, const UDenseJob*, uint32_t n_jobs, uint32_t n_blocks, const uint32_t*, const uint32_t*, uint32_t lo_doc, uint32_t*, float*) {
    log_launch("k_union_dense_write", {n_jobs, n_blocks, lo_doc});
    no_device("k_union_dense_write");
}
void launch_dict_scan_wide(hipStream_t, uint32_t char_bytes, const DictProbeW*, const uint32_t*, uint32_t probe_base, uint32_t n_probes, const uint32_t*, const void*, const void*,
                           uint32_t num_terms, uint32_t*, uint32_t out_cap, DictMatch*) {
    log_launch("k_dict_scan_wide", {char_bytes, probe_base, n_probes, num_terms, out_cap});
    no_device("k_dict_scan_wide");
}
// VQ_STUB_DICT_SCAN=1 (tools/host_profile.py; the pre-pass batch of tests/native/launch_plan_driver.py): exact / prefix probes answered by a plain
// loop, so that requests with prefix leaves get through compile_batch (exec.cpp; run_fuzzy_probes in prepass.cpp) without a GPU.  The sanitizer test leaves it off: there every launcher throws.
void launch_dict_scan(hipStream_t, const DictProbe* probes, uint32_t probe_base, uint32_t n_probes, const uint32_t* off, const uint16_t* chars, const uint16_t* low_chars,
                      uint32_t num_terms, uint32_t* out_count, uint32_t out_cap, DictMatch* out) {
    log_launch("k_dict_scan", {probe_base, n_probes, num_terms, out_cap});
    if (!std::getenv("VQ_STUB_DICT_SCAN")) no_device("k_dict_scan");
    for (uint32_t p = 0; p < n_probes; ++p) {
        const DictProbe& P = probes[p];
        if (P.max_d != 0) no_device("k_dict_scan (the stub's loop answers distance 0 only)");
        for (uint32_t t = 0; t < num_terms; ++t) {
            const uint32_t n = off[t + 1] - off[t];
            if ((P.flags & 2u) ? n < P.m : n != P.m) continue;
            bool eq = true;
            for (uint32_t i = 0; i < P.m && eq; ++i) eq = chars[off[t] + i] == P.query[i];
            if (!eq) continue;
            uint32_t info = 0;
            if (P.lm != 0xFFFFFFFFu) {  // lower-cased hit against the lower-cased term: a prefix match is n - lm insertions away
                bool starts = n >= P.lm;
                for (uint32_t i = 0; i < P.lm && starts; ++i) starts = low_chars[off[t] + i] == P.lquery[i];
                const uint32_t d = starts ? std::min<uint32_t>(n - P.lm, 255u) : 255u;
                info = d | (d << 8) | (uint32_t(starts) << 16);
            }
            const uint32_t pos = (*out_count)++;
            if (pos < out_cap) out[pos] = DictMatch{probe_base + p, t, info};
        }
    }
}
void launch_loc_gather(hipStream_t, const LocRow*, uint32_t n_rows, const uint32_t*, uint32_t*) {
    log_launch("k_loc_gather", {n_rows});
    no_device("k_loc_gather");
}
void launch_loc_expand(hipStream_t, bool write, const LocJob*, uint32_t n_jobs, const uint32_t*, uint32_t n, uint32_t*, unsigned long long*) {
    log_launch("k_loc_expand", {write, n_jobs, n});
    no_device("k_loc_expand");
}
void launch_loc_compact(hipStream_t, const LocJob*, uint32_t n_jobs, const unsigned long long*, uint32_t*, float*, uint32_t*) {
    log_launch("k_loc_compact", {n_jobs});
    no_device("k_loc_compact");
}
size_t seg_sort_u32(void*, size_t, const uint32_t*, uint32_t*, uint32_t n, uint32_t nseg, const uint32_t*, const uint32_t*, hipStream_t) {
    log_launch("seg_sort_u32", {n, nseg});
    no_device("seg_sort_u32");
    return 0;
}
size_t seg_sort_u64(void*, size_t, const unsigned long long*, unsigned long long*, uint32_t n, uint32_t nseg, const uint32_t*, const uint32_t*, hipStream_t) {
    log_launch("seg_sort_u64", {n, nseg});
    no_device("seg_sort_u64");
    return 0;
}
void launch_b1n_map(hipStream_t, const B1nJob*, uint32_t n_jobs, const uint32_t*, uint32_t*, float*, B1nResult*) {
    log_launch("k_b1n_map", {n_jobs});
    no_device("k_b1n_map");
}
void launch_explain(hipStream_t, uint32_t n_docs, const ExQuery*, const uint32_t*, const uint32_t*, const ExOp*, const uint16_t*, const ExList*, const DColBoost*, uint32_t*) {
    log_launch("k_explain", {n_docs});
    no_device("k_explain");
}
// With VQ_STUB_DICT_SCAN=1 the regex scan is answered on the host as well, walking the very tables k_dict_regex would read and writing DictMatch
// records through the same counter-and-capacity protocol: what the host side made of a pattern — DFA, premultiplied states, class tables,
// alphabet — is then checked end to end without a GPU.
void launch_dict_regex(hipStream_t, uint32_t char_bytes, bool small_tables, const RegexProbeD* probes, const uint16_t* pool, const uint32_t* alpha, uint32_t n_alpha,
                       uint32_t probe_base, uint32_t n_probes, const uint32_t* off, const void* chars, uint32_t num_terms, uint32_t* out_count, uint32_t out_cap,
                       DictMatch* out) {
    log_launch("k_dict_regex", {char_bytes, small_tables, n_alpha, probe_base, n_probes, num_terms, out_cap});
    if (!std::getenv("VQ_STUB_DICT_SCAN")) {
        no_device("k_dict_regex");
        return;
    }
    for (uint32_t p = 0; p < n_probes; ++p) {
        const RegexProbeD& P = probes[p];
        const uint64_t lds = uint64_t(regex_words16(P.n_next, n_alpha)) * 2 + uint64_t(n_alpha) * 4;
        if (lds > (small_tables ? vqregex::kLdsTableBytesSmall : vqregex::kLdsTableBytes) + 32u || P.start >= P.n_next)
            throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_dict_regex (stub): a probe whose tables the kernel would refuse");
        const uint16_t* next = pool + P.tab_off;
        const uint16_t* ascii = next + P.n_next;
        const uint16_t* acls = ascii + 128;
        for (uint32_t t = 0; t < num_terms; ++t) {
            uint32_t state = P.start;
            for (uint32_t i = off[t]; i < off[t + 1]; ++i) {
                const uint32_t cp = char_bytes == 4 ? static_cast<const uint32_t*>(chars)[i] : static_cast<const uint16_t*>(chars)[i];
                uint32_t c;
                if (cp < 128u) c = ascii[cp];
                else {
                    uint32_t lo = 0, hi = n_alpha;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (alpha[mid] < cp) lo = mid + 1u;
                        else hi = mid;
                    }
                    c = lo < n_alpha ? acls[lo] : 0u;
                }
                if (state + c >= P.n_next) throw vqreq::VelociError(vqreq::ERR_DEVICE, "k_dict_regex (stub): a transition outside the table");
                state = next[state + c];
            }
            if (state >= P.first_accept) {
                const uint32_t pos = (*out_count)++;
                if (pos < out_cap) out[pos] = DictMatch{probe_base + p, t, 0u};
            }
        }
    }
}
}  // namespace vq

extern "C" void vq_stub_fail_launches_after(long k) { vq::stub_set_fail_after(k); }
