// Posterior sample paths of the d = 4 discrete smoothers by backward simulation (cgp_sample4.hpp; cgp_smoother_sample): rts for the linear
// model, eks and sgp_smoother (the literal sum over any d = 4 sigma-point set) for the chirp / La Scala LCD models.
#include "cgp_sample4.hpp"
#include "cgp_dispatch.hpp"
namespace cgp {
int dispatch_sample4(int method, int model_id, const SampleIO& io, const ModelArgs& ma, hipStream_t st) {
    const bool lcd = model_id == CGP_M_HARMONIC_LCD || model_id == CGP_M_LASCALA_LCD;
    if (method == CGP_S_EKS && model_id == CGP_M_LINEAR) return hip_rc(launch_sample4<EksElement<LinearDisc<4>>>(io, ma, st));
    if (method == CGP_S_EKS && lcd) return hip_rc(launch_sample4<EksElement<HarmonicLCD<1>>>(io, ma, st));
    if (method == CGP_S_SGP && lcd) return hip_rc(launch_sample4<SgpsElement<HarmonicLCD<1>>>(io, ma, st));
    return CGP_E_UNSUPPORTED;
}
}  // namespace cgp
