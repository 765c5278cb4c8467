// TEST INFRASTRUCTURE — the launcher behind vq_debug_col_boost (veloci_amd/csrc/kernels.hip) for the host builds that stub the device layer (see
// hip_stub.cpp): no device, so the hook declines with -1 after its argument handling and its parse of the boost have run.  Never linked into
// the product library.
#include "../../veloci_amd/csrc/engine.hpp"

namespace vq {
int debug_col_boost(DColBoost, const float*, uint32_t, const uint32_t*, uint32_t, const uint32_t*, const float*, uint32_t, float*, float*) { return -1; }
}  // namespace vq
