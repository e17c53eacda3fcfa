// cgp_cd_ekf_nll_grad: the continuous-discrete EKF's NLL with its exact gradient by forward tangents through the RK4 stages and the
// update -- the instantiation of cgp_tangent4_cd.hpp.  With CGP_SKIP_MISSING it hands the launch to the GAPS instantiation of
// cgp_inst_gaps4_tangent_cd.hip, with CGP_RK4_SUBSTEPS (and either) to those of cgp_inst_substeps4_tangent_cd.hip.
#include "cgp_tangent4_cd.hpp"
using namespace cgp;

extern "C" int cgp_cd_ekf_nll_grad(cgp_ctx* ctx, const cgp_model* model, const cgp_init* init, double dt,
                                   const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                                   const double* dirs, int32_t n_dir, double* nll, double* grad, uint32_t flags, void* stream) {
    if (!ctx) return CGP_E_ARG;
    TangentIO io{};
    ModelArgs ma;
    const Verdict prepared = prepare_tangent({"cgp_cd_ekf_nll_grad", false, false, true}, model, nullptr, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T,
                                             dirs, n_dir, nll, grad, nullptr, flags, io, ma);
    return launch_on(ctx, prepared, kLaunchLocked, [&]() -> Verdict {
        const hipStream_t st = (hipStream_t)stream;
        if (flags & CGP_RK4_SUBSTEPS_MASK) return hip_rc(launch_cd_ekf4_tangent_substeps(io, ma, (flags & CGP_SKIP_MISSING) != 0, st));
        return hip_rc((flags & CGP_SKIP_MISSING) ? launch_cd_ekf4_tangent_gaps(io, ma, st) : launch_cd_ekf4_tangent<false>(io, ma, st));
    });
}
