// cgp_sgp_nll_grad and cgp_sgp_nll_fisher: the sigma-point filter's NLL with its exact gradient by forward tangents through the scan, and
// with the Fisher information of its Gaussian innovations model along the caller's directions -- the instantiations of
// cgp_tangent4_sigma.hpp.  With CGP_SKIP_MISSING both hand the launch to the GAPS instantiations of cgp_inst_gaps4_tangent_sgp.hip.
// cgp_sgp_nll_grad with a CGP_M_HARMONIC_SDE model is the continuous-discrete sigma-point filter's (cgp_tangent4_cd_sigma.hpp): its launch
// goes to cgp_inst_tangent4_cd_sgp.hip or cgp_inst_gaps4_tangent_cd_sgp.hip.
#define CGP_COOP4_HELPERS_ONLY          // the cooperative EKF and the EKF tangent kernel live in their own units
#define CGP_TANGENT4_IO_ONLY
#include "cgp_tangent4_sigma.hpp"
using namespace cgp;

static_assert(kFisherMaxDir <= kSgpMaxDir, "the Fisher form runs as one launch: every direction needs an owner lane");

extern "C" int cgp_sgp_nll_grad(cgp_ctx* ctx, const cgp_model* model, const cgp_sigma* sigma, const cgp_init* init, double dt,
                                const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                                const double* dirs, int32_t n_dir, double* nll, double* grad, uint32_t flags, void* stream) {
    if (!ctx) return CGP_E_ARG;
    TangentIO io{};
    ModelArgs ma;
    const Verdict prepared = prepare_tangent({"cgp_sgp_nll_grad", true, false}, model, sigma, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T,
                                             dirs, n_dir, nll, grad, nullptr, flags, io, ma);
    return launch_on(ctx, prepared, kLaunchLocked, [&]() -> Verdict {
        const hipStream_t st = (hipStream_t)stream;
        if (model->model_id == CGP_M_HARMONIC_SDE)       // cd_sgp_filter's form (prepare_tangent has checked the model's shape; substeps: ma.substeps)
            return hip_rc((flags & CGP_SKIP_MISSING) ? launch_cd_sgp4_tangent_gaps(io, ma, st) : launch_cd_sgp4_tangent_plain(io, ma, st));
        return hip_rc((flags & CGP_SKIP_MISSING) ? launch_sgp4_tangent_gaps(io, ma, false, st) : launch_sgp4_tangent(io, ma, st));
    });
}

extern "C" int cgp_sgp_nll_fisher(cgp_ctx* ctx, const cgp_model* model, const cgp_sigma* sigma, const cgp_init* init, double dt,
                                  const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                                  const double* dirs, int32_t n_dir, double* nll, double* grad, double* fisher, uint32_t flags, void* stream) {
    if (!ctx) return CGP_E_ARG;
    TangentIO io{};
    ModelArgs ma;
    const Verdict prepared = prepare_tangent({"cgp_sgp_nll_fisher", true, true}, model, sigma, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T,
                                             dirs, n_dir, nll, grad, fisher, flags, io, ma);
    return launch_on(ctx, prepared, kLaunchLocked, [&]() -> Verdict {
        const hipStream_t st = (hipStream_t)stream;
        return hip_rc((flags & CGP_SKIP_MISSING) ? launch_sgp4_tangent_gaps(io, ma, true, st) : launch_sgp4_tangent<true>(io, ma, st));
    });
}
