// TEST INFRASTRUCTURE — the wide dictionary scan's launcher for the stubbed device layer (see hip_stub.cpp): it throws like every other stubbed
// launcher (with VQ_STUB_NOOP_LAUNCH=1 it does nothing).  Linked next to hip_stub.cpp into the CPU sanitizer and host-stub builds only.
#include <cstdlib>
#include <string>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
void launch_dict_scan_wide(hipStream_t, uint32_t, const DictProbeW*, const uint32_t*, uint32_t, uint32_t, const uint32_t*, const void*, const void*, uint32_t, uint32_t*,
                           uint32_t, DictMatch*) {
    if (std::getenv("VQ_STUB_NOOP_LAUNCH")) return;
    throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: k_dict_scan_wide"));
}
}  // namespace vq
