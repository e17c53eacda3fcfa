// cgp_sgp_nll_grad and cgp_sgp_nll_fisher: the sigma-point filter's NLL with its exact gradient by forward tangents through the scan, and
// with the Fisher information of its Gaussian innovations model along the caller's directions -- the instantiations of
// cgp_tangent4_sigma.hpp.  With CGP_SKIP_MISSING both hand the launch to the GAPS instantiations of cgp_inst_gaps4_tangent_sgp.hip.
#define CGP_COOP4_HELPERS_ONLY          // the cooperative EKF and the EKF tangent kernel live in their own units
#define CGP_TANGENT4_IO_ONLY
#include "cgp_tangent4_sigma.hpp"
using namespace cgp;

static_assert(kFisherMaxDir <= kSgpMaxDir, "the Fisher form runs as one launch: every direction needs an owner lane");

extern "C" int cgp_sgp_nll_grad(cgp_ctx* ctx, const cgp_model* model, const cgp_sigma* sigma, const cgp_init* init, double dt,
                                const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                                const double* dirs, int32_t n_dir, double* nll, double* grad, uint32_t flags, void* stream) {
    TangentIO io;
    ModelArgs ma;
    const int rc = tangent_args(ctx, {"cgp_sgp_nll_grad", true, false}, model, sigma, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T,
                                dirs, n_dir, nll, grad, nullptr, flags, io, ma);
    if (rc != CGP_OK || io.B == 0) return rc;
    if (B > 0x7fffffffLL) return fail(ctx, CGP_E_UNSUPPORTED, "cgp_sgp_nll_grad runs one workgroup per trial: B must be < 2^31");
    if (flags & CGP_SKIP_MISSING) return tangent_launch(ctx, [&] { return launch_sgp4_tangent_gaps(io, ma, false, (hipStream_t)stream); });
    return tangent_launch(ctx, [&] { return launch_sgp4_tangent(io, ma, (hipStream_t)stream); });
}

extern "C" int cgp_sgp_nll_fisher(cgp_ctx* ctx, const cgp_model* model, const cgp_sigma* sigma, const cgp_init* init, double dt,
                                  const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                                  const double* dirs, int32_t n_dir, double* nll, double* grad, double* fisher, uint32_t flags, void* stream) {
    TangentIO io;
    ModelArgs ma;
    const int rc = tangent_args(ctx, {"cgp_sgp_nll_fisher", true, true}, model, sigma, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T,
                                dirs, n_dir, nll, grad, fisher, flags, io, ma);
    if (rc != CGP_OK || io.B == 0) return rc;
    if (B > 0x7fffffffLL) return fail(ctx, CGP_E_UNSUPPORTED, "cgp_sgp_nll_fisher runs one workgroup per trial: B must be < 2^31");
    if (flags & CGP_SKIP_MISSING) return tangent_launch(ctx, [&] { return launch_sgp4_tangent_gaps(io, ma, true, (hipStream_t)stream); });
    return tangent_launch(ctx, [&] { return launch_sgp4_tangent<true>(io, ma, (hipStream_t)stream); });
}
