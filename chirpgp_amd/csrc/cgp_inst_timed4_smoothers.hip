// The TIMED instantiations (include/chirpgp_hip_timed.h: the step from row t + 1 to row t runs over dts[t + 1]) of the matrix-core smoothers
// cd_eks and cd_sgp_smoother at d = 4 (cgp_mfma4_cd.hpp: cd4_mfma_smoother_walk), in a translation unit of their own, so that
// cgp_inst_mfma4.hip compiles to what it compiled to.  Built like it (Makefile).
#define CGP_COOP4_HELPERS_ONLY
#define CGP_NO_UNTIMED_CD_EKS      // the untimed cd_eks kernels stay in the units they are built in
#include "cgp_mfma4.hpp"
#include "cgp_mfma4_sigma.hpp"
#include "cgp_mfma4_cd.hpp"
namespace cgp {
int dispatch_smoother_mfma4_cdeks_timed(const SmootherIO& io, const ModelArgs& ma, hipStream_t st) { return launch_cdeks4_mfma_timed(io, ma, st); }
int dispatch_smoother_mfma4_cdsgp_timed(const SmootherIO& io, const ModelArgs& ma, hipStream_t st) { return launch_cdsgps4_mfma_timed<HarmonicSDE<1>>(io, ma, st); }
}  // namespace cgp
