// The GAPS instantiations (CGP_SKIP_MISSING: a NaN measurement is a missing sample) of the one-wavefront-per-trial matrix-core filters at
// d = 4 -- sgp_filter (cgp_mfma4_sigma.hpp), cd_sgp_filter and cd_ekf (cgp_mfma4_cd.hpp) -- in a translation unit of their own, so that the
// units of the unflagged kernels compile to what they compiled to.  Built like cgp_inst_mfma4_sgpf.hip (Makefile): the two sigma-point
// filters want the plain-fma polynomial steps; cd_ekf measured 3 - 4 % slower with them in its unflagged form and takes them here all the
// same -- its flagged form is not worth a third unit until somebody measures it.
#define CGP_COOP4_HELPERS_ONLY
#define CGP_HORNER_PLAIN
#include "cgp_mfma4.hpp"
#include "cgp_mfma4_sigma.hpp"
#include "cgp_mfma4_cd.hpp"
namespace cgp {
int dispatch_filter_mfma4_sgp_gaps(const FilterIO& io, const ModelArgs& ma, hipStream_t st) { return launch_sgp4_mfma<HarmonicLCD<1>, true>(io, ma, st); }
int dispatch_filter_mfma4_cdsgp_gaps(const FilterIO& io, const ModelArgs& ma, hipStream_t st) { return launch_cdsgp4_mfma<HarmonicSDE<1>, true>(io, ma, st); }
int dispatch_filter_mfma4_cdekf_gaps(const FilterIO& io, const ModelArgs& ma, hipStream_t st) { return launch_cdekf4_mfma<true>(io, ma, st); }
}  // namespace cgp
