// cgp_sgp_nll_grad on the d = 4 chirp / La Scala SDE (CGP_M_HARMONIC_SDE): the continuous-discrete sigma-point filter's NLL with its exact
// gradient by forward tangents through the RK4 stages of the sigma-point moment ODE and the update -- the unflagged instantiation of
// cgp_tangent4_cd_sigma.hpp.  CGP_RK4_SUBSTEPS is a trip count of the kernel (ma.substeps), so this unit and the GAPS one
// (cgp_inst_gaps4_tangent_cd_sgp.hip) are all there is.  cgp_sgp_nll_grad (cgp_inst_tangent4_sgp.hip) checks the arguments and hands the
// launch over.
#define CGP_COOP4_HELPERS_ONLY
#define CGP_TANGENT4_IO_ONLY
#include "cgp_tangent4_cd_sigma.hpp"
namespace cgp {
hipError_t launch_cd_sgp4_tangent_plain(const TangentIO& io, const ModelArgs& ma, hipStream_t stream) {
    return launch_cd_sgp4_tangent<false>(io, ma, stream);
}
}  // namespace cgp
