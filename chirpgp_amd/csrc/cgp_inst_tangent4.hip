// cgp_ekf_nll_grad and cgp_ekf_nll_fisher: the EKF's NLL with its exact gradient by forward tangents through the scan, and with the
// Fisher information of its Gaussian innovations model along the caller's directions -- the instantiations of cgp_tangent4.hpp.  With
// CGP_SKIP_MISSING both hand the launch to the GAPS instantiations of cgp_inst_gaps4_tangent.hip.
#include "cgp_tangent4.hpp"
using namespace cgp;

extern "C" int cgp_ekf_nll_grad(cgp_ctx* ctx, const cgp_model* model, const cgp_init* init, double dt,
                                const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                                const double* dirs, int32_t n_dir, double* nll, double* grad, uint32_t flags, void* stream) {
    TangentIO io;
    ModelArgs ma;
    const int rc = tangent_args(ctx, {"cgp_ekf_nll_grad", false, false}, model, nullptr, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T,
                                dirs, n_dir, nll, grad, nullptr, flags, io, ma);
    if (rc != CGP_OK || io.B == 0) return rc;
    if (flags & CGP_SKIP_MISSING) return tangent_launch(ctx, [&] { return launch_ekf4_tangent_gaps(io, ma, false, (hipStream_t)stream); });
    return tangent_launch(ctx, [&] { return launch_ekf4_tangent(io, ma, (hipStream_t)stream); });
}

extern "C" int cgp_ekf_nll_fisher(cgp_ctx* ctx, const cgp_model* model, const cgp_init* init, double dt,
                                  const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                                  const double* dirs, int32_t n_dir, double* nll, double* grad, double* fisher, uint32_t flags, void* stream) {
    TangentIO io;
    ModelArgs ma;
    const int rc = tangent_args(ctx, {"cgp_ekf_nll_fisher", false, true}, model, nullptr, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T,
                                dirs, n_dir, nll, grad, fisher, flags, io, ma);
    if (rc != CGP_OK || io.B == 0) return rc;
    if ((B + (64 / n_dir) - 1) / (64 / n_dir) > 0x7fffffffLL) return fail(ctx, CGP_E_UNSUPPORTED, "cgp_ekf_nll_fisher: too many trials for one grid");
    if (flags & CGP_SKIP_MISSING) return tangent_launch(ctx, [&] { return launch_ekf4_tangent_gaps(io, ma, true, (hipStream_t)stream); });
    return tangent_launch(ctx, [&] { return launch_ekf4_fisher(io, ma, (hipStream_t)stream); });
}
