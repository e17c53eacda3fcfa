// Lane-cooperative d = 4 kernels (chirp / La Scala models): EKF (cgp_coop4.hpp) and the sigma-point filters and
// continuous-discrete smoother (cgp_coop4_sigma.hpp), the continuous-discrete EKF / EKS (cgp_coop4_cd.hpp) -- what CGP_DPP_KERNEL asks
// for, and what takes the launches the matrix-core kernels do not (cgp_route.hpp).
#include "cgp_coop4_cd.hpp"
namespace cgp {
int dispatch_filter_coop4(const FilterIO& io, const ModelArgs& ma, hipStream_t st) { return launch_ekf4_coop(io, ma, st); }
int dispatch_filter_coop4_sgp(const FilterIO& io, const ModelArgs& ma, hipStream_t st) { return launch_sgp4_coop<HarmonicLCD<1>>(io, ma, st); }
int dispatch_filter_coop4_cdsgp(const FilterIO& io, const ModelArgs& ma, hipStream_t st) { return launch_cdsgp4_coop<HarmonicSDE<1>>(io, ma, st); }
int dispatch_smoother_coop4_cdsgp(const SmootherIO& io, const ModelArgs& ma, hipStream_t st) { return launch_cdsgps4_coop<HarmonicSDE<1>>(io, ma, st); }
int dispatch_filter_coop4_cdekf(const FilterIO& io, const ModelArgs& ma, hipStream_t st) { return launch_cdekf4_coop(io, ma, st); }
int dispatch_smoother_coop4_cdeks(const SmootherIO& io, const ModelArgs& ma, hipStream_t st) { return launch_cdeks4_coop(io, ma, st); }
}  // namespace cgp
