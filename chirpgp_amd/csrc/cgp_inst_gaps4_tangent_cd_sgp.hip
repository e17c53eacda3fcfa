// The GAPS instantiation (CGP_SKIP_MISSING: a NaN measurement is a missing sample) of the continuous-discrete sigma-point filter's tangent
// kernel (cgp_tangent4_cd_sigma.hpp: cd_sgp4_tangent_kernel<true>), with CGP_RK4_SUBSTEPS or without, in a translation unit of its own as the
// other tangent kernels' are.
#define CGP_COOP4_HELPERS_ONLY
#define CGP_TANGENT4_IO_ONLY
#include "cgp_tangent4_cd_sigma.hpp"
namespace cgp {
hipError_t launch_cd_sgp4_tangent_gaps(const TangentIO& io, const ModelArgs& ma, hipStream_t stream) {
    return launch_cd_sgp4_tangent<true>(io, ma, stream);
}
}  // namespace cgp
