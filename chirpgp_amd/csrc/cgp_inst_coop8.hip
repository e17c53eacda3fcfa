// Lane-cooperative kernels in the 8 x 8 tile layout (cgp_coop8.hpp): harmonic chirp models with two or three harmonics.
// The sigma-point filter and the smoothers take their polynomial steps as the compiler's own fma (C5's filter 10.68 -> 10.58 ms, its
// smoother 4.69 -> 4.57 ms; profiles/r04_ab_series.txt); the EKF of the same header measured 1.7 % slower with it and is instantiated
// in cgp_inst_coop8_ekf.hip with the inline-asm step.
#define CGP_COOP4_HELPERS_ONLY
#define CGP_HORNER_PLAIN
#include "cgp_coop8.hpp"
namespace cgp {
int dispatch_filter_coop8_sgp(int n_harm, const FilterIO& io, const ModelArgs& ma, hipStream_t st) {
    switch (n_harm) {
    case 2: return launch_sgp8_coop<2>(io, ma, st);
    case 3: return launch_sgp8_coop<3>(io, ma, st);
    default: return CGP_E_UNSUPPORTED;
    }
}
int dispatch_smoother_coop8_linear(int method, int d, const SmootherIO& io, const SmootherLaunch& host, const ModelArgs& ma, hipStream_t st) {
    if (method != CGP_S_EKS && method != CGP_S_SGP) return CGP_E_UNSUPPORTED;
    const bool sg = method == CGP_S_SGP;
    switch (d) {
    case 5: return hip_rc(sg ? launch_coop8_smoother<SgpsElement<LinearDisc<5>>>(io, host, ma, st) : launch_coop8_smoother<EksElement<LinearDisc<5>>>(io, host, ma, st));
    case 6: return hip_rc(sg ? launch_coop8_smoother<SgpsElement<LinearDisc<6>>>(io, host, ma, st) : launch_coop8_smoother<EksElement<LinearDisc<6>>>(io, host, ma, st));
    case 7: return hip_rc(sg ? launch_coop8_smoother<SgpsElement<LinearDisc<7>>>(io, host, ma, st) : launch_coop8_smoother<EksElement<LinearDisc<7>>>(io, host, ma, st));
    case 8: return hip_rc(sg ? launch_coop8_smoother<SgpsElement<LinearDisc<8>>>(io, host, ma, st) : launch_coop8_smoother<EksElement<LinearDisc<8>>>(io, host, ma, st));
    default: return CGP_E_UNSUPPORTED;
    }
}
// (the sigma-point elements of the harmonic models in their collapsed form only: coop8_smoother_harm_ok, cgp_route.hpp)
int dispatch_smoother_coop8_harm(int method, int n_harm, const SmootherIO& io, const SmootherLaunch& host, const ModelArgs& ma, hipStream_t st) {
    if (method != CGP_S_EKS && method != CGP_S_SGP) return CGP_E_UNSUPPORTED;
    const bool sg = method == CGP_S_SGP;
    switch (n_harm) {
    case 2: return hip_rc(sg ? launch_coop8_smoother<SgpsElement<HarmonicLCD<2>, true>>(io, host, ma, st) : launch_coop8_smoother<EksElement<HarmonicLCD<2>>>(io, host, ma, st));
    case 3: return hip_rc(sg ? launch_coop8_smoother<SgpsElement<HarmonicLCD<3>, true>>(io, host, ma, st) : launch_coop8_smoother<EksElement<HarmonicLCD<3>>>(io, host, ma, st));
    default: return CGP_E_UNSUPPORTED;
    }
}
}  // namespace cgp
