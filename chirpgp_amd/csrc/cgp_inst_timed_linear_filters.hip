// Timed calls (include/chirpgp_hip_timed.h) on the linear SDE (drift A u, constant dispersion), d = 1..8: the generic filter kernels on
// TimedPredict (cgp_steps.hpp), with and without CGP_RK4_SUBSTEPS, in a unit of their own so that the untimed units compile to what they did.
#include "cgp_dispatch.hpp"
namespace cgp {
int dispatch_filter_sde_linear_timed(int method, int key, bool wave, bool sub, const FilterIO& io, const ModelArgs& ma, hipStream_t st) {
    switch (key) {
    case 1: return filter_sde_timed<LinearSDE<1>>(method, wave, sub, io, ma, st);
    case 2: return filter_sde_timed<LinearSDE<2>>(method, wave, sub, io, ma, st);
    case 3: return filter_sde_timed<LinearSDE<3>>(method, wave, sub, io, ma, st);
    case 4: return filter_sde_timed<LinearSDE<4>>(method, wave, sub, io, ma, st);
    case 5: return filter_sde_timed<LinearSDE<5>>(method, wave, sub, io, ma, st);
    case 6: return filter_sde_timed<LinearSDE<6>>(method, wave, sub, io, ma, st);
    case 7: return filter_sde_timed<LinearSDE<7>>(method, wave, sub, io, ma, st);
    case 8: return filter_sde_timed<LinearSDE<8>>(method, wave, sub, io, ma, st);
    default: return CGP_E_UNSUPPORTED;
    }
}
}  // namespace cgp
