// Leaf top-n of the batched suggest on the device: the reference's streaming top-n loop (search_field.rs:322-333 + sort.rs:25-34) run over a
// probe's matches instead of copying every match back.
//
//   grouping     k_dict_scan appends the matches of all probes of a batch to one DictMatch array in no order.  k_topn_keys turns every record
//                into the key  rank(probe) << 32 | term  with `info` as its value, rocPRIM's radix sort brings them into (probe, ascending
//                term) order — the FST stream order the reference's callback sees — and k_topn_bounds writes every probe's segment.  The host
//                ranks the full-route probes first, so their records are one contiguous piece at the front (seg[2 * n_ranks] = its length).
//   k_dict_topn  one wave64 (a one-wave workgroup) per top-n probe walks its segment 64 matches per step.  The loop is order dependent: a hit
//                below `worst` is skipped; a hit that finds the buffer at top_n + 200 entries first sorts it (score desc, id desc), truncates it
//                to top_n and raises `worst` to the last kept score, and is then pushed whatever its score.  Which of several tied hits survive
//                depends on where these events fall, so the walk repeats them exactly: passing lanes are appended by prefix rank until the
//                buffer is full, the next passing lane fires the event, and the lanes behind it are tested again against the new `worst`.
//   scores       never computed here.  A hit's class is 2 * distance + prefix_matches; the host ranks the 512 classes by the f32 score ITS
//                arithmetic gives them (equal floats share a rank) and uploads `ord` = 0xFFFF - rank.  score desc, id desc is then one
//                descending 64-bit key  ord << 41 | term << 9 | class.
//   LDS          the buffer: 8 bytes per entry, the launch's largest top_n + 200 rounded up to a power of two (at most 2048 entries, 16 KiB)
//   packing      k_topn_offsets gives probe p room for min(its matches, top_n + 200) entries behind those of the probes before it, so what is
//                copied back never exceeds the matches there are
//   output       per probe the number of entries and (class << 32 | term) per entry in BUFFER order: after an event the kept top_n in sorted
//                order, then the later pushes in id order — the order the host's stable sort depends on.
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "kernel_common.hpp"
#include "kernels.hpp"

namespace vq {

__global__ __launch_bounds__(256) void k_topn_keys(const DictMatch* __restrict__ recs, uint32_t n, const uint32_t* __restrict__ rank_of, uint32_t n_ranks,
                                                   unsigned long long* __restrict__ keys, uint32_t* __restrict__ infos) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const VQ_GLOBAL uint32_t* w = as_global(reinterpret_cast<const uint32_t*>(recs)) + 3ull * i;
    const uint32_t probe = w[0], term = w[1], info = w[2];
    // (a probe number outside the table cannot come from the scan kernels; it gets the rank behind all others, which no segment serves)
    const uint32_t rank = probe < n_ranks ? as_global(rank_of)[probe] : n_ranks;
    keys[i] = ((unsigned long long)rank << 32) | term;
    infos[i] = info;
}

// seg[2r], seg[2r + 1]: the records of rank r in the sorted keys (both zeroed before: a rank without a record keeps an empty segment);
// seg[2 * n_ranks]: the records of the ranks below n_full (the full-route piece)
__global__ __launch_bounds__(256) void k_topn_bounds(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t n_ranks, uint32_t n_full, uint32_t* __restrict__ seg) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = (uint32_t)(keys[i] >> 32);
    const bool first = i == 0u || (uint32_t)(keys[i - 1u] >> 32) != r;
    const uint32_t next = i + 1u < n ? (uint32_t)(keys[i + 1u] >> 32) : 0xFFFFFFFFu;
    if (r < n_ranks) {
        if (first) seg[2u * r] = i;
        if (next != r) seg[2u * r + 1u] = i + 1u;
    }
    if (r < n_full && next >= n_full) seg[2u * n_ranks] = i + 1u;
}

// out_off[p]: entries the probes before p may write (each min(matches, top_n + 200)); out_off[n]: the total.  One wave.
__global__ __launch_bounds__(64) void k_topn_offsets(const TopnProbeD* __restrict__ probes, uint32_t n, const uint32_t* __restrict__ seg, uint32_t* __restrict__ out_off) {
    uint32_t running = 0u;
    for (uint32_t base = 0u; base < n; base += 64u) {
        const uint32_t j = base + lane_id();
        uint32_t len = 0u;
        if (j < n) {
            const uint32_t rank = probes[j].rank, room = probes[j].top_n + kTopnSlack, matches = seg[2u * rank + 1u] - seg[2u * rank];
            len = matches < room ? matches : room;
        }
        uint32_t total;
        const uint32_t before = wave_excl_scan_u32(len, &total);
        if (j < n) out_off[j] = running + before;
        running += total;
    }
    if (lane_id() == 0u) out_off[n] = running;
}

// bitonic sort of buf[0, m) descending, m a power of two, by the 64 lanes of the one wave of the workgroup
__device__ __forceinline__ void topn_sort_desc(unsigned long long* buf, uint32_t m) {
    const uint32_t lane = lane_id();
    for (uint32_t size = 2; size <= m; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = lane; t < (m >> 1); t += 64u) {
                const uint32_t i = ((t & ~(stride - 1u)) << 1) | (t & (stride - 1u));
                const uint32_t j = i + stride;
                const bool desc = (i & size) == 0;
                const unsigned long long a = buf[i], b = buf[j];
                if ((a < b) == desc) {
                    buf[i] = b;
                    buf[j] = a;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(64) void k_dict_topn(const TopnProbeD* __restrict__ probes, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ infos,
                                                 const uint32_t* __restrict__ seg, const uint16_t* __restrict__ class_ord, uint32_t lds_entries,
                                                 const uint32_t* __restrict__ out_offs, uint32_t* __restrict__ out_n, unsigned long long* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long topn_buf[];
    const VQ_CONST TopnProbeD* P = as_const<TopnProbeD>(probes + blockIdx.x);
    const uint32_t top_n = P->top_n, lev = P->lev, check_prefix = P->check_prefix, out_off = out_offs[blockIdx.x];
    const uint32_t begin = seg[2u * P->rank], end = seg[2u * P->rank + 1u];
    const uint32_t limit = top_n + kTopnSlack;
    uint32_t m = 256u;  // the power of two the full buffer is sorted as
    while (m < limit) m <<= 1;
    if (top_n == 0u || m > lds_entries) {  // (uniform; the host never sends such a probe)
        if (threadIdx.x == 0u) out_n[blockIdx.x] = 0u;
        return;
    }
    const uint32_t lane = lane_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t size = 0u;   // entries of the buffer (uniform)
    uint32_t worst = 0u;  // `ord` of worst_score (uniform): f32::MIN, below every class, before the first event
    for (uint32_t base = begin; base < end; base += 64u) {
        const uint32_t i = base + lane;
        const bool valid = i < end;
        unsigned long long key = 0ull;
        uint32_t ord = 0u;
        if (valid) {
            const uint32_t term = (uint32_t)keys[i], info = as_global(infos)[i];
            const uint32_t osa = info & 0xFFu, plain = (info >> 8) & 0xFFu, starts = (info >> 16) & 1u;
            const uint32_t d = osa <= lev ? osa : plain;  // the scoring automaton's answer, else its Levenshtein fallback (search_field.rs:691-732)
            const uint32_t c = 2u * d + (check_prefix & starts);
            ord = as_global(class_ord)[c];
            key = ((unsigned long long)ord << 41) | ((unsigned long long)term << 9) | c;
        }
        unsigned long long pending = __ballot(valid);  // lanes of this step the loop has not decided yet (uniform)
        while (pending) {
            const unsigned long long pass = __ballot(valid && ord >= worst) & pending;  // (score < worst_score: skipped)
            if (!pass) break;
            const uint32_t room = limit - size;
            if (room == 0u) {  // the event, fired by the first passing lane: it passed the OLD worst and is pushed after the cut
                for (uint32_t k = limit + lane; k < m; k += 64u) topn_buf[k] = 0ull;  // (below every key: ord > 0)
                __syncthreads();
                topn_sort_desc(topn_buf, m);
                worst = (uint32_t)(topn_buf[top_n - 1u] >> 41);
                __syncthreads();
                const uint32_t first = (uint32_t)__builtin_ctzll(pass);
                if (lane == first) topn_buf[top_n] = key;
                size = top_n + 1u;
                pending &= ~((2ull << first) - 1ull);  // (the lanes in front of it failed the old worst: they fail the new one)
                continue;
            }
            const uint32_t mine = (uint32_t)__popcll(pass & below);
            const bool in_pass = (pass >> lane) & 1ull;
            if (in_pass && mine < room) topn_buf[size + mine] = key;
            const uint32_t n_pass = (uint32_t)__popcll(pass);
            if (n_pass <= room) {
                size += n_pass;
                pending = 0ull;  // (worst has not changed: the others stay skipped)
            } else {  // the buffer is full now: the lanes behind the last one taken go round again
                const unsigned long long last = __ballot(in_pass && mine == room - 1u);
                size = limit;
                pending &= ~((2ull << (uint32_t)__builtin_ctzll(last)) - 1ull);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u) out_n[blockIdx.x] = size;
    for (uint32_t k = lane; k < size; k += 64u) {
        const unsigned long long key = topn_buf[k];
        out[(size_t)out_off + k] = ((key & 0x1FFull) << 32) | ((key >> 9) & 0xFFFFFFFFull);
    }
}

static uint32_t topn_key_end_bit(uint32_t n_ranks) {  // bits of rank << 32 | term that can be set (ranks 0 .. n_ranks, the last for strays)
    uint32_t bits = 1;
    while (bits < 32u && (1ull << bits) <= n_ranks) ++bits;
    return 32u + bits;
}

size_t dict_topn_sort_tmp_bytes(uint32_t n, uint32_t n_ranks) {
    size_t bytes = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, static_cast<const unsigned long long*>(nullptr), static_cast<unsigned long long*>(nullptr),
                                                   static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), n, 0u, topn_key_end_bit(n_ranks), hipStream_t(nullptr));
    return e == hipSuccess ? bytes : size_t(-1);
}

bool launch_dict_topn_group(hipStream_t st, const DictMatch* recs, uint32_t n, const uint32_t* rank_of, uint32_t n_ranks, uint32_t n_full, unsigned long long* keys_in,
                            unsigned long long* keys_sorted, uint32_t* infos_in, uint32_t* infos_sorted, void* tmp, size_t tmp_bytes, uint32_t* seg) {
    if (hipMemsetAsync(seg, 0, (2u * size_t(n_ranks) + 1u) * 4u, st) != hipSuccess) return false;
    if (!n) return true;
    const uint32_t blocks = (n + 255u) / 256u;
    hipLaunchKernelGGL(k_topn_keys, dim3(blocks), dim3(256), 0, st, recs, n, rank_of, n_ranks, keys_in, infos_in);
    size_t bytes = tmp_bytes;
    if (rocprim::radix_sort_pairs(tmp, bytes, static_cast<const unsigned long long*>(keys_in), keys_sorted, static_cast<const uint32_t*>(infos_in), infos_sorted, n, 0u,
                                  topn_key_end_bit(n_ranks), st) != hipSuccess)
        return false;
    hipLaunchKernelGGL(k_topn_bounds, dim3(blocks), dim3(256), 0, st, keys_sorted, n, n_ranks, n_full, seg);
    return true;
}

uint32_t dict_topn_lds_entries(uint32_t max_top_n) {
    uint32_t m = 256u;
    while (m < max_top_n + kTopnSlack) m <<= 1;
    return m;
}

void launch_dict_topn(hipStream_t st, const TopnProbeD* probes, uint32_t n_probes, uint32_t max_top_n, const unsigned long long* keys, const uint32_t* infos,
                      const uint32_t* seg, const uint16_t* class_ord, uint32_t* out_off, uint32_t* out_n, unsigned long long* out) {
    if (!n_probes) return;
    const uint32_t entries = dict_topn_lds_entries(max_top_n);
    hipLaunchKernelGGL(k_topn_offsets, dim3(1), dim3(64), 0, st, probes, n_probes, seg, out_off);
    hipLaunchKernelGGL(k_dict_topn, dim3(n_probes), dim3(64), size_t(entries) * 8u, st, probes, keys, infos, seg, class_ord, entries, out_off, out_n, out);
}

// self-check (tests): k_dict_topn on one crafted stream of (term, class) in stream order -> the final buffer.  0, or -1 without a device
int debug_dict_topn(const uint32_t* terms, const uint32_t* classes, uint32_t n, uint32_t top_n, const uint16_t* class_ord_host, uint32_t* out_terms, uint32_t* out_classes,
                    uint32_t* out_n) {
    std::vector<unsigned long long> keys(n ? n : 1u), outv(top_n + kTopnSlack);
    std::vector<uint32_t> infos(n ? n : 1u);
    for (uint32_t i = 0; i < n; ++i) {  // distance class >> 1 from the automaton (lev 255 takes it as it is), the prefix bit as `starts`
        keys[i] = terms[i];
        infos[i] = (classes[i] >> 1) | ((classes[i] >> 1) << 8) | ((classes[i] & 1u) << 16);
    }
    const TopnProbeD P{0u, top_n, 255u, 1u, {0u, 0u, 0u, 0u}};
    const uint32_t seg[2] = {0u, n};
    unsigned long long *d_keys = nullptr, *d_out = nullptr;
    uint32_t *d_infos = nullptr, *d_seg = nullptr, *d_n = nullptr, *d_off = nullptr;
    uint16_t* d_ord = nullptr;
    TopnProbeD* d_p = nullptr;
    uint32_t got = 0;
    bool ok = hipMalloc(&d_keys, keys.size() * 8) == hipSuccess && hipMalloc(&d_out, outv.size() * 8) == hipSuccess && hipMalloc(&d_infos, infos.size() * 4) == hipSuccess &&
              hipMalloc(&d_seg, sizeof seg) == hipSuccess && hipMalloc(&d_off, 8) == hipSuccess && hipMalloc(&d_n, 4) == hipSuccess && hipMalloc(&d_ord, 512 * 2) == hipSuccess && hipMalloc(&d_p, sizeof P) == hipSuccess;
    ok = ok && hipMemcpy(d_keys, keys.data(), keys.size() * 8, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_infos, infos.data(), infos.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_seg, seg, sizeof seg, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_ord, class_ord_host, 512 * 2, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_p, &P, sizeof P, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_dict_topn(nullptr, d_p, 1, top_n, d_keys, d_infos, d_seg, d_ord, d_off, d_n, d_out);
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(&got, d_n, 4, hipMemcpyDeviceToHost) == hipSuccess && got <= outv.size() &&
             hipMemcpy(outv.data(), d_out, outv.size() * 8, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d_keys);
    (void)hipFree(d_out);
    (void)hipFree(d_infos);
    (void)hipFree(d_seg);
    (void)hipFree(d_off);
    (void)hipFree(d_n);
    (void)hipFree(d_ord);
    (void)hipFree(d_p);
    if (!ok) return -1;
    for (uint32_t k = 0; k < got; ++k) {
        out_terms[k] = uint32_t(outv[k]);
        out_classes[k] = uint32_t(outv[k] >> 32);
    }
    *out_n = got;
    return 0;
}

}  // namespace vq
