// The SUB instantiations (CGP_RK4_SUBSTEPS: n RK4 steps of dt / n between two measurements) of the one-wavefront-per-trial matrix-core
// filters cd_ekf and cd_sgp_filter at d = 4 (cgp_mfma4_cd.hpp), with and without GAPS, in a translation unit of their own, so that the units
// of the unflagged kernels compile to what they compiled to.  Built like cgp_inst_gaps4_sigma.hip (Makefile).
#define CGP_COOP4_HELPERS_ONLY
#define CGP_HORNER_PLAIN
#include "cgp_mfma4.hpp"
#include "cgp_mfma4_sigma.hpp"
#include "cgp_mfma4_cd.hpp"
namespace cgp {
int dispatch_filter_mfma4_cdekf_substeps(bool gaps, const FilterIO& io, const ModelArgs& ma, hipStream_t st) {
    return gaps ? launch_cdekf4_mfma_substeps<true>(io, ma, st) : launch_cdekf4_mfma_substeps<false>(io, ma, st);
}
int dispatch_filter_mfma4_cdsgp_substeps(bool gaps, const FilterIO& io, const ModelArgs& ma, hipStream_t st) {
    return gaps ? launch_cdsgp4_mfma_substeps<HarmonicSDE<1>, true>(io, ma, st) : launch_cdsgp4_mfma_substeps<HarmonicSDE<1>, false>(io, ma, st);
}
}  // namespace cgp
