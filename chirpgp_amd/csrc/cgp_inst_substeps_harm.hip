// CGP_RK4_SUBSTEPS on the harmonic chirp SDE (model_chirp, model_harmonic_chirp, model_lascala), n_harm = 1..3: the generic kernels on
// SubstepPredict / SubstepSmooth (cgp_steps.hpp), in a unit of their own so that cgp_inst_sde_harm.hip compiles to what it did.
#include "cgp_dispatch.hpp"
namespace cgp {
int dispatch_filter_sde_harm_substeps(int method, int key, bool wave, const FilterIO& io, const ModelArgs& ma, hipStream_t st) {
    switch (key) {
    case 1: return filter_sde_substeps<HarmonicSDE<1>>(method, wave, io, ma, st);
    case 2: return filter_sde_substeps<HarmonicSDE<2>>(method, wave, io, ma, st);
    case 3: return filter_sde_substeps<HarmonicSDE<3>>(method, wave, io, ma, st);
    default: return CGP_E_UNSUPPORTED;
    }
}
int dispatch_smoother_sde_harm_substeps(int method, int key, const SmootherIO& io, const ModelArgs& ma, hipStream_t st) {
    switch (key) {
    case 1: return smoother_sde_substeps<HarmonicSDE<1>>(method, io, ma, st);
    case 2: return smoother_sde_substeps<HarmonicSDE<2>>(method, io, ma, st);
    case 3: return smoother_sde_substeps<HarmonicSDE<3>>(method, io, ma, st);
    default: return CGP_E_UNSUPPORTED;
    }
}
}  // namespace cgp
