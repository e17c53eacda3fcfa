// cgp_ekf_nll_grad and cgp_ekf_nll_fisher: the EKF's NLL with its exact gradient by forward tangents through the scan, and with the
// Fisher information of its Gaussian innovations model along the caller's directions -- the instantiations of cgp_tangent4.hpp.  With
// CGP_SKIP_MISSING both hand the launch to the GAPS instantiations of cgp_inst_gaps4_tangent.hip.
#include "cgp_tangent4.hpp"
using namespace cgp;

extern "C" int cgp_ekf_nll_grad(cgp_ctx* ctx, const cgp_model* model, const cgp_init* init, double dt,
                                const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                                const double* dirs, int32_t n_dir, double* nll, double* grad, uint32_t flags, void* stream) {
    if (!ctx) return CGP_E_ARG;
    TangentIO io{};
    ModelArgs ma;
    const Verdict prepared = prepare_tangent({"cgp_ekf_nll_grad", false, false}, model, nullptr, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T,
                                             dirs, n_dir, nll, grad, nullptr, flags, io, ma);
    return launch_on(ctx, prepared, kLaunchLocked, [&]() -> Verdict {
        const hipStream_t st = (hipStream_t)stream;
        return hip_rc((flags & CGP_SKIP_MISSING) ? launch_ekf4_tangent_gaps(io, ma, false, st) : launch_ekf4_tangent(io, ma, st));
    });
}

extern "C" int cgp_ekf_nll_fisher(cgp_ctx* ctx, const cgp_model* model, const cgp_init* init, double dt,
                                  const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                                  const double* dirs, int32_t n_dir, double* nll, double* grad, double* fisher, uint32_t flags, void* stream) {
    if (!ctx) return CGP_E_ARG;
    TangentIO io{};
    ModelArgs ma;
    const Verdict prepared = prepare_tangent({"cgp_ekf_nll_fisher", false, true}, model, nullptr, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T,
                                             dirs, n_dir, nll, grad, fisher, flags, io, ma);
    return launch_on(ctx, prepared, kLaunchLocked, [&]() -> Verdict {
        const hipStream_t st = (hipStream_t)stream;
        return hip_rc((flags & CGP_SKIP_MISSING) ? launch_ekf4_tangent_gaps(io, ma, true, st) : launch_ekf4_fisher(io, ma, st));
    });
}
