// The TIMED instantiations (include/chirpgp_hip_timed.h: each step integrates over its own interval dts[t]) of the one-wavefront-per-trial
// matrix-core filters cd_ekf and cd_sgp_filter at d = 4 (cgp_mfma4_cd.hpp), with and without GAPS and SUB, in a translation unit of their
// own, so that the units of the untimed kernels compile to what they compiled to.  Built like cgp_inst_substeps4.hip (Makefile).
#define CGP_COOP4_HELPERS_ONLY
#define CGP_NO_UNTIMED_CD_EKS      // the untimed cd_eks kernels stay in the units they are built in
#define CGP_HORNER_PLAIN
#include "cgp_mfma4.hpp"
#include "cgp_mfma4_sigma.hpp"
#include "cgp_mfma4_cd.hpp"
namespace cgp {
int dispatch_filter_mfma4_cdekf_timed(bool gaps, bool sub, const FilterIO& io, const ModelArgs& ma, hipStream_t st) {
    if (sub) return gaps ? launch_cdekf4_mfma_timed<true, true>(io, ma, st) : launch_cdekf4_mfma_timed<false, true>(io, ma, st);
    return gaps ? launch_cdekf4_mfma_timed<true, false>(io, ma, st) : launch_cdekf4_mfma_timed<false, false>(io, ma, st);
}
int dispatch_filter_mfma4_cdsgp_timed(bool gaps, bool sub, const FilterIO& io, const ModelArgs& ma, hipStream_t st) {
    using SM = HarmonicSDE<1>;
    if (sub) return gaps ? launch_cdsgp4_mfma_timed<SM, true, true>(io, ma, st) : launch_cdsgp4_mfma_timed<SM, false, true>(io, ma, st);
    return gaps ? launch_cdsgp4_mfma_timed<SM, true, false>(io, ma, st) : launch_cdsgp4_mfma_timed<SM, false, false>(io, ma, st);
}
}  // namespace cgp
