// The GAPS instantiation (CGP_SKIP_MISSING: a NaN measurement is a missing sample) of the continuous-discrete EKF's tangent kernel
// (cgp_tangent4_cd.hpp: cd_ekf4_tangent_kernel<true>) in a translation unit of its own, as the other tangent kernels' gated forms are.
// cgp_cd_ekf_nll_grad checks the arguments and hands a flagged launch over.
#include "cgp_tangent4_cd.hpp"
namespace cgp {
hipError_t launch_cd_ekf4_tangent_gaps(const TangentIO& io, const ModelArgs& ma, hipStream_t stream) {
    return launch_cd_ekf4_tangent<true>(io, ma, stream);
}
}  // namespace cgp
