// The GAPS instantiations (CGP_SKIP_MISSING: a NaN measurement is a missing sample) of the sigma-point filter's tangent kernel
// (cgp_tangent4_sigma.hpp: sgp4_tangent_kernel<kFisher, true>), gradient and Fisher form, in a translation unit of their own, so that the unit
// of the unflagged kernels (cgp_inst_tangent4_sgp.hip) compiles to what it compiled to.  cgp_sgp_nll_grad and cgp_sgp_nll_fisher check the
// arguments and hand a flagged launch over.
#define CGP_COOP4_HELPERS_ONLY
#define CGP_TANGENT4_IO_ONLY
#include "cgp_tangent4_sigma.hpp"
namespace cgp {
hipError_t launch_sgp4_tangent_gaps(const TangentIO& io, const ModelArgs& ma, bool fisher, hipStream_t stream) {
    return fisher ? launch_sgp4_tangent<true, true>(io, ma, stream) : launch_sgp4_tangent<false, true>(io, ma, stream);
}
}  // namespace cgp
