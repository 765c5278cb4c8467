// TEST INFRASTRUCTURE — the per-shape probe scan's launcher for the stubbed device layer (see hip_stub.cpp): it throws like every other stubbed
// launcher (with VQ_STUB_NOOP_LAUNCH=1 it does nothing).  Linked next to hip_stub.cpp into the CPU sanitizer and host-stub builds only.
#include <cstdlib>
#include <string>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
void launch_scan_probe_shape(hipStream_t, uint32_t, uint32_t, uint32_t, uint32_t, const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t,
                             unsigned long long*, unsigned long long*) {
    if (std::getenv("VQ_STUB_NOOP_LAUNCH")) return;
    throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: k_scan_probe"));
}
size_t scan_probe_lds_bytes(uint32_t, uint32_t, uint32_t, uint32_t) { return 0; }
uint32_t debug_probe_occupancy(uint32_t, size_t) { return 0; }
}  // namespace vq
