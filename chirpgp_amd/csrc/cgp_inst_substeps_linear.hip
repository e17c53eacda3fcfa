// CGP_RK4_SUBSTEPS on the linear SDE (drift A u, constant dispersion), d = 1..8: the generic kernels on SubstepPredict / SubstepSmooth
// (cgp_steps.hpp), in a unit of their own so that cgp_inst_sde_linear.hip compiles to what it did.
#include "cgp_dispatch.hpp"
namespace cgp {
int dispatch_filter_sde_linear_substeps(int method, int key, bool wave, const FilterIO& io, const ModelArgs& ma, hipStream_t st) {
    switch (key) {
    case 1: return filter_sde_substeps<LinearSDE<1>>(method, wave, io, ma, st);
    case 2: return filter_sde_substeps<LinearSDE<2>>(method, wave, io, ma, st);
    case 3: return filter_sde_substeps<LinearSDE<3>>(method, wave, io, ma, st);
    case 4: return filter_sde_substeps<LinearSDE<4>>(method, wave, io, ma, st);
    case 5: return filter_sde_substeps<LinearSDE<5>>(method, wave, io, ma, st);
    case 6: return filter_sde_substeps<LinearSDE<6>>(method, wave, io, ma, st);
    case 7: return filter_sde_substeps<LinearSDE<7>>(method, wave, io, ma, st);
    case 8: return filter_sde_substeps<LinearSDE<8>>(method, wave, io, ma, st);
    default: return CGP_E_UNSUPPORTED;
    }
}
int dispatch_smoother_sde_linear_substeps(int method, int key, const SmootherIO& io, const ModelArgs& ma, hipStream_t st) {
    switch (key) {
    case 1: return smoother_sde_substeps<LinearSDE<1>>(method, io, ma, st);
    case 2: return smoother_sde_substeps<LinearSDE<2>>(method, io, ma, st);
    case 3: return smoother_sde_substeps<LinearSDE<3>>(method, io, ma, st);
    case 4: return smoother_sde_substeps<LinearSDE<4>>(method, io, ma, st);
    case 5: return smoother_sde_substeps<LinearSDE<5>>(method, io, ma, st);
    case 6: return smoother_sde_substeps<LinearSDE<6>>(method, io, ma, st);
    case 7: return smoother_sde_substeps<LinearSDE<7>>(method, io, ma, st);
    case 8: return smoother_sde_substeps<LinearSDE<8>>(method, io, ma, st);
    default: return CGP_E_UNSUPPORTED;
    }
}
}  // namespace cgp
