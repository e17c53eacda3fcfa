// Timed calls (include/chirpgp_hip_timed.h) on the harmonic chirp SDE (model_chirp, model_harmonic_chirp, model_lascala), n_harm = 1..3: the generic smoother kernels on
// TimedSmooth (cgp_steps.hpp), with and without CGP_RK4_SUBSTEPS, in a unit of their own so that the untimed units compile to what they did.
#include "cgp_dispatch.hpp"
namespace cgp {
int dispatch_smoother_sde_harm_timed(int method, int key, bool wave, bool sub, const SmootherIO& io, const ModelArgs& ma, hipStream_t st) {
    switch (key) {
    case 1: return smoother_sde_timed<HarmonicSDE<1>>(method, wave, sub, io, ma, st);
    case 2: return smoother_sde_timed<HarmonicSDE<2>>(method, wave, sub, io, ma, st);
    case 3: return smoother_sde_timed<HarmonicSDE<3>>(method, wave, sub, io, ma, st);
    default: return CGP_E_UNSUPPORTED;
    }
}
}  // namespace cgp
