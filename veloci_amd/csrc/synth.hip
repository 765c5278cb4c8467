// Synthetic-corpus input generation (veloci_amd/synth.py), not the query path: membership of every doc of a range in one probe list, fused.
// Bit for bit the torch definition in synth.py: h32(key, d) = splitmix64_finalizer(d * GOLD + mix(key)) >> 32, a doc is in the list when
// h32(key, d) < thr or (shared) h32(shared_key, d) < shared_thr.  Built into veloci_amd/libveloci_synth.so, loaded by synth.py.
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void k_synth_member(uint64_t lo, uint64_t n, uint64_t key_mix, uint64_t thr, uint64_t shared_mix, uint64_t shared_thr, uint8_t* out) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t g = (lo + i) * 0x9E3779B97F4A7C15ull;
        const bool in = (mix64(g + key_mix) >> 32) < thr || (mix64(g + shared_mix) >> 32) < shared_thr;
        out[i] = in ? 1 : 0;
    }
}

}  // namespace

// out[i] = 1 when doc lo + i is a member (shared_thr = 0: no shared part), on `stream`; returns a hipError_t
extern "C" int vq_synth_member(uint64_t lo, uint64_t n, uint64_t key_mix, uint64_t thr, uint64_t shared_mix, uint64_t shared_thr, uint8_t* out,
                               void* stream) {
    if (n == 0) return hipSuccess;
    const unsigned block = 256;
    const uint64_t want = (n + block - 1) / block;
    const unsigned grid = unsigned(want < 65536 ? want : 65536);
    hipLaunchKernelGGL(k_synth_member, dim3(grid), dim3(block), 0, static_cast<hipStream_t>(stream), lo, n, key_mix, thr, shared_mix, shared_thr, out);
    return int(hipGetLastError());
}
