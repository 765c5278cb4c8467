// TEST INFRASTRUCTURE — the dense union's launchers for the stubbed device layer (see hip_stub.cpp): they throw like every other stubbed
// launcher (with VQ_STUB_NOOP_LAUNCH=1 they do nothing).  Linked next to hip_stub.cpp into the CPU sanitizer and host-stub builds only.
#include <cstdlib>
#include <string>

#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
static void stubbed(const char* what) {
    if (std::getenv("VQ_STUB_NOOP_LAUNCH")) return;
    throw vqreq::VelociError(vqreq::ERR_DEVICE, std::string("device layer stubbed: ") + what);
}
void launch_union_dense_scatter(hipStream_t, const UDenseList*, uint32_t, uint64_t, const UDenseJob*, uint32_t*, uint32_t, uint32_t) { stubbed("k_union_dense_scatter"); }
void launch_union_dense_count(hipStream_t, const UDenseJob*, uint32_t, uint32_t, const uint32_t*, uint32_t*, uint32_t*, UDenseResult*) { stubbed("k_union_dense_count"); }
void launch_union_dense_write(hipStream_t, const UDenseJob*, uint32_t, uint32_t, const uint32_t*, const uint32_t*, uint32_t, uint32_t*, float*) { stubbed("k_union_dense_write"); }
}  // namespace vq
