// Text ranking of the batched highlight on the device: the step of resolve_token_hits_to_text_id (search_field.rs:550-639) that turns a part's
// matched tokens into ranked texts, cut to the page before anything comes back.
//
//   k_text_best    one wave64 per row descriptor (slot, row start, row length, score bits): a piece of at most kTextRankSplit values of one
//                  matched token's tokens_to_text_id row.  Lanes stream the row's text ids 64 at a time (coalesced) and issue a no-return
//                  atomicMax of the token's score bits on best[slot][text].  The scores are finite and > 0, so their f32 bit patterns order
//                  as u32 and the maximum does not depend on the order of the atomics; 0 means "no matched token in this text".
//   k_text_select  one workgroup of 1024 threads per slot.  A radix select over the score bits, 8 bits per pass from the top byte down
//                  (a 256-bin LDS histogram; a wave whose live lanes all fall into one bin adds their count once), finds the bit pattern of
//                  the top_n-th best touched text; its first pass also counts the touched texts.  Then every wave takes one contiguous piece
//                  of the array: it counts its texts equal to the threshold, the counts are summed over the waves in front of it, and a
//                  second walk in text order (ballot + prefix count) writes every text above the threshold and the first top_n - above
//                  texts equal to it, in ascending text id.  The pairs above the threshold are written in no order: the host sorts the page.
//   output         per slot (text, score bits) pairs, at most top_n of them, their number and the number of touched texts
#include <vector>

#include "kernel_common.hpp"
#include "kernels.hpp"

namespace vq {

constexpr uint32_t kSelectThreads = 1024, kSelectWaves = kSelectThreads / 64;

__global__ __launch_bounds__(256) void k_text_best(const TextRowD* __restrict__ rows, uint32_t n_rows, const uint32_t* __restrict__ vals, uint32_t num_texts,
                                                   uint32_t* __restrict__ best) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= n_rows) return;  // (uniform per wave)
    const VQ_CONST TextRowD* R = as_const<TextRowD>(rows + r);
    const unsigned long long start = R->start;
    const uint32_t len = R->len, bits = R->bits;
    uint32_t* mine = best + (size_t)R->slot * num_texts;
    const VQ_GLOBAL uint32_t* v = as_global(vals) + start;
    for (uint32_t i = lane_id(); i < len; i += 64u) {
        const uint32_t text = v[i];
        if (text < num_texts) atomicMax(mine + text, bits);
    }
}

__global__ __launch_bounds__(kSelectThreads) void k_text_select(const uint32_t* __restrict__ best, uint32_t num_texts, const uint32_t* __restrict__ top_ns, uint32_t out_stride,
                                                                uint32_t* __restrict__ out_counts, uint32_t* __restrict__ out_pairs) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_want, s_done, s_above_at;
    __shared__ uint32_t wave_eq[kSelectWaves];
    const uint32_t slot = blockIdx.x, tid = threadIdx.x;
    const VQ_GLOBAL uint32_t* b = as_global(best) + (size_t)slot * num_texts;
    uint32_t top_n = top_ns[slot];
    if (top_n > out_stride) top_n = out_stride;  // (the host never sends such a slot)
    uint32_t* pairs = out_pairs + (size_t)slot * out_stride * 2u;
    if (tid == 0u) {
        s_prefix = 0u;
        s_want = top_n;
        s_done = 0u;
        s_above_at = 0u;
    }
    uint32_t touched = 0u;
    // radix select: after the pass over byte k, s_prefix holds the top 4 - k bytes of the top_n-th best value and s_want its rank among the
    // values that share them
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256u) hist[tid] = 0u;
        __syncthreads();
        const uint32_t prefix = s_prefix, mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (uint32_t base = 0u; base < num_texts; base += kSelectThreads) {  // (uniform trip count: hist_add's ballots see whole waves)
            const uint32_t i = base + tid;
            const uint32_t v = i < num_texts ? b[i] : 0u;
            hist_add(hist, v != 0u && (v & mask) == prefix, (v >> shift) & 0xFFu);
        }
        __syncthreads();
        if (tid == 0u) {
            uint32_t want = s_want, seen = 0u, bin = 256u;
            while (bin > 0u && seen + hist[bin - 1u] < want) seen += hist[--bin];
            if (bin == 0u) {  // fewer candidates than wanted (only in the first pass: fewer touched texts than top_n): everything is taken
                s_done = 1u;
                s_want = seen;
            } else {
                s_prefix = prefix | ((bin - 1u) << shift);
                s_want = want - seen;
            }
            if (shift == 24) {
                uint32_t total = 0u;
                for (uint32_t k = 0u; k < 256u; ++k) total += hist[k];
                out_counts[2u * slot + 1u] = total;
                hist[0] = total;  // (read back below, behind the barrier)
            }
        }
        __syncthreads();
        if (shift == 24) touched = hist[0];
        if (s_done) break;
        __syncthreads();  // (hist[0] is cleared by the next pass)
    }
    const bool all = s_done != 0u;
    // all: every touched text (there are s_want <= top_n); else the texts above `thr` and the first `want_eq` equal to it in text order
    const uint32_t thr = all ? 0u : s_prefix, want_eq = all ? 0u : s_want, above = all ? 0u : top_n - want_eq;
    const uint32_t wave = tid >> 6, lane = lane_id();
    const uint32_t piece = (num_texts + kSelectWaves - 1u) / kSelectWaves;
    const uint32_t lo = wave * piece < num_texts ? wave * piece : num_texts, hi = lo + piece < num_texts ? lo + piece : num_texts;
    uint32_t eq_before = 0u;
    if (!all) {
        uint32_t mine = 0u;
        for (uint32_t base = lo; base < hi; base += 64u) {
            const uint32_t i = base + lane;
            mine += (uint32_t)__popcll(__ballot(i < hi && b[i] == thr));
        }
        if (lane == 0u) wave_eq[wave] = mine;
        __syncthreads();
        for (uint32_t w = 0u; w < wave; ++w) eq_before += wave_eq[w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t base = lo; base < hi; base += 64u) {
        const uint32_t i = base + lane;
        const uint32_t v = i < hi ? b[i] : 0u;
        const bool is_above = v > thr;
        if (is_above) {  // (no order among them: at most `above` of them, or `touched` <= top_n when everything is taken)
            const uint32_t at = atomicAdd(&s_above_at, 1u);
            if (at < top_n) {
                pairs[2u * at] = i;
                pairs[2u * at + 1u] = v;
            }
        }
        if (!all && eq_before < want_eq) {  // (uniform per wave)
            const bool is_eq = i < hi && v == thr;
            const unsigned long long m = __ballot(is_eq);
            const uint32_t rank = eq_before + (uint32_t)__popcll(m & below);
            if (is_eq && rank < want_eq) {
                pairs[2u * (above + rank)] = i;
                pairs[2u * (above + rank) + 1u] = v;
            }
            eq_before += (uint32_t)__popcll(m);
        }
    }
    if (tid == 0u) out_counts[2u * slot] = touched < top_n ? touched : top_n;
}

void launch_text_best(hipStream_t st, const TextRowD* rows, uint32_t n_rows, const uint32_t* vals, uint32_t num_texts, uint32_t* best) {
    if (!n_rows) return;
    hipLaunchKernelGGL(k_text_best, dim3((n_rows + 3u) / 4u), dim3(256), 0, st, rows, n_rows, vals, num_texts, best);
}

void launch_text_select(hipStream_t st, const uint32_t* best, uint32_t num_texts, uint32_t n_slots, const uint32_t* top_ns, uint32_t out_stride, uint32_t* out_counts,
                        uint32_t* out_pairs) {
    if (!n_slots) return;
    hipLaunchKernelGGL(k_text_select, dim3(n_slots), dim3(kSelectThreads), 0, st, best, num_texts, top_ns, out_stride, out_counts, out_pairs);
}

}  // namespace vq
