// The posterior Cramer-Rao sums (cgp_pcrlb_sums): instantiations.
#include "cgp_pcrlb.hpp"

namespace cgp {
int dispatch_pcrlb(int model_id, int key, const PcrlbIO& io, const ModelArgs& ma, hipStream_t st) {
    if (model_id == CGP_M_LINEAR) {
        switch (key) {
        case 1: return launch_pcrlb<LinearDisc<1>>(io, ma, st);
        case 2: return launch_pcrlb<LinearDisc<2>>(io, ma, st);
        case 3: return launch_pcrlb<LinearDisc<3>>(io, ma, st);
        case 4: return launch_pcrlb<LinearDisc<4>>(io, ma, st);
        case 5: return launch_pcrlb<LinearDisc<5>>(io, ma, st);
        case 6: return launch_pcrlb<LinearDisc<6>>(io, ma, st);
        case 7: return launch_pcrlb<LinearDisc<7>>(io, ma, st);
        case 8: return launch_pcrlb<LinearDisc<8>>(io, ma, st);
        default: return CGP_E_UNSUPPORTED;
        }
    }
    switch (key) {
    case 1: return launch_pcrlb<HarmonicLCD<1>>(io, ma, st);
    case 2: return launch_pcrlb<HarmonicLCD<2>>(io, ma, st);
    case 3: return launch_pcrlb<HarmonicLCD<3>>(io, ma, st);
    default: return CGP_E_UNSUPPORTED;
    }
}
}  // namespace cgp
