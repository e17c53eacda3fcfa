// The GAPS instantiations (CGP_SKIP_MISSING: a NaN measurement is a missing sample) of the EKF's tangent kernel (cgp_tangent4.hpp:
// ekf4_tangent_kernel<kSlots, true>) -- the gradient form and the Fisher form's four row sizes -- in a translation unit of their own, so
// that the unit of the unflagged kernels (cgp_inst_tangent4.hip) compiles to what it compiled to.  cgp_ekf_nll_grad and cgp_ekf_nll_fisher
// check the arguments and hand a flagged launch over.
#include "cgp_tangent4.hpp"
namespace cgp {
hipError_t launch_ekf4_tangent_gaps(const TangentIO& io, const ModelArgs& ma, bool fisher, hipStream_t stream) {
    return fisher ? launch_ekf4_fisher<true>(io, ma, stream) : launch_ekf4_tangent<0, true>(io, ma, stream);
}
}  // namespace cgp
