// The d = 4 matrix-core EKF for records with gaps (CGP_SKIP_MISSING; cgp_mfma4.hpp: ekf4_gaps_kernel) in a translation unit of its own, so
// that the units of the headline kernels (cgp_inst_ekf4.hip, cgp_inst_ekf4_x4.hip) compile to what they compiled to.  Flags (Makefile): VGPR-form
// MFMA results, the default scheduling strategy and no machine-level loop-invariant code motion, as for the one-trial kernel's unit -- with
// it the 64-bit literals of the wide and the checked step's polynomials are hoisted out of the chunk loop and overflow the scalar file
// here too (101 scalar spills against 2, 241 VGPRs against 169).
#define CGP_COOP4_HELPERS_ONLY
#define CGP_EKF4_GAPS_KERNELS
#define CGP_HORNER_PLAIN
#include "cgp_mfma4.hpp"
namespace cgp {
int dispatch_filter_mfma4_gaps(const FilterIO& io, const ModelArgs& ma, hipStream_t st) { return launch_ekf4_gaps(io, ma, st); }
}  // namespace cgp
