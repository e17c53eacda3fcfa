// cgp_cd_ekf_nll_grad: the continuous-discrete EKF's NLL with its exact gradient by forward tangents through the RK4 stages and the
// update -- the instantiation of cgp_tangent4_cd.hpp.  With CGP_SKIP_MISSING it hands the launch to the GAPS instantiation of
// cgp_inst_gaps4_tangent_cd.hip.
#include "cgp_tangent4_cd.hpp"
using namespace cgp;

extern "C" int cgp_cd_ekf_nll_grad(cgp_ctx* ctx, const cgp_model* model, const cgp_init* init, double dt,
                                   const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                                   const double* dirs, int32_t n_dir, double* nll, double* grad, uint32_t flags, void* stream) {
    TangentIO io;
    ModelArgs ma;
    const int rc = tangent_args(ctx, {"cgp_cd_ekf_nll_grad", false, false, true}, model, nullptr, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T,
                                dirs, n_dir, nll, grad, nullptr, flags, io, ma);
    if (rc != CGP_OK || io.B == 0) return rc;
    if (B > (0x7fffffffLL * 64) / n_dir) return fail(ctx, CGP_E_UNSUPPORTED, "cgp_cd_ekf_nll_grad: too many lanes (B n_dir) for one grid");
    if (flags & CGP_SKIP_MISSING) return tangent_launch(ctx, [&] { return launch_cd_ekf4_tangent_gaps(io, ma, (hipStream_t)stream); });
    return tangent_launch(ctx, [&] { return launch_cd_ekf4_tangent<false>(io, ma, (hipStream_t)stream); });
}
