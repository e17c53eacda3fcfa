// cgp_cd_ekf_nll_grad with CGP_RK4_SUBSTEPS (n RK4 steps of dt / n between two measurements): the continuous-discrete EKF's tangent kernel
// with its four-stage loop run n times per sample, with and without GAPS.  A kernel template of its own, in a translation unit of its own:
// cd_ekf4_tangent_kernel (cgp_tangent4_cd.hpp) is left as it is, text and code.  Everything but the substep loop is that kernel's: the
// stage function cd_ekf4_tangent_stage, the layout (one lane per (trial, direction)), the update tangent_update<GAPS>.  ma.dt is the
// substep h = dt / n, divided once on the host (cgp_args.hpp); h carries no tangent, so the directions are the plain call's.
#include "cgp_tangent4_cd.hpp"
namespace cgp {

template <bool GAPS>
__global__ void __launch_bounds__(64) cd_ekf4_tangent_substeps_kernel(TangentIO io, ModelArgs ma) {
    const int64_t gi = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (gi >= io.B * io.n_dir) return;                                    // (a partial wavefront runs with a partial EXEC mask)
    const int64_t trial = gi / io.n_dir;
    const int dir = (int)(gi - trial * io.n_dir);

    HarmonicSDE<1> model;
    model.setup(ma.params + trial * ma.param_stride, ma.model_id);
    const double* __restrict__ dp = io.dirs + gi * kCdDirDoubles;
    CdTangentModel q;
    q.lam = model.lam; q.gam = model.gam; q.fs = model.fs; q.dlam = dp[0]; q.dgam = dp[1];
    {
        const double* __restrict__ gm = ma.gamma + trial * ma.gamma_stride;
        int k = 0;
        CGP_UNROLL for (int i = 0; i < 4; i++) CGP_UNROLL for (int j = 0; j <= i; j++) { q.G[k] = gm[i * 4 + j]; q.dG[k] = dp[2 + k]; k++; }
    }
    const double dXi = dp[12];
    const double dt = ma.dt, dt6 = ma.dt / 6.0;                           // h and h / 6
    const int nsub = ma.substeps;
    double h[4];
    CGP_UNROLL for (int i = 0; i < 4; i++) h[i] = io.H[trial * io.H_stride + i];
    const double Xi = io.Xi[trial * io.Xi_stride];

    double m[4], dm[4], P[10], dP[10];
    CGP_UNROLL for (int i = 0; i < 4; i++) { m[i] = io.m0[trial * io.m0_stride + i]; dm[i] = dp[13 + i]; }
    {
        const double* __restrict__ p0 = io.P0 + trial * io.P0_stride;
        int k = 0;
        CGP_UNROLL for (int i = 0; i < 4; i++) CGP_UNROLL for (int j = 0; j <= i; j++) { P[k] = p0[i * 4 + j]; dP[k] = dp[17 + k]; k++; }
    }
    double nll = 0.0, dnll = 0.0;
    const double* __restrict__ rec = io.record(trial);

    for (int64_t t0 = 0; t0 < io.T; t0 += 8) {
        double yb[8];
        CGP_UNROLL for (int k = 0; k < 8; k++) yb[k] = (t0 + k < io.T) ? rec[t0 + k] : 0.0;
        const int n = (io.T - t0 < 8) ? (int)(io.T - t0) : 8;
        for (int k = 0; k < n; k++) {
            const double y = yb[k];
            // ---- nsub RK4 steps of (m, P) with its tangent, in place: x + h (k1 + 2 k2 + 2 k3 + k4) / 6
#pragma unroll 1
            for (int j = 0; j < nsub; j++) {
                double tm[4], tdm[4], tP[10], tdP[10], am[4], adm[4], aP[10], adP[10];
                CGP_UNROLL for (int i = 0; i < 4; i++) { tm[i] = m[i]; tdm[i] = dm[i]; am[i] = 0.0; adm[i] = 0.0; }
                CGP_UNROLL for (int i = 0; i < 10; i++) { tP[i] = P[i]; tdP[i] = dP[i]; aP[i] = 0.0; adP[i] = 0.0; }
#pragma unroll 1
                for (int stage = 0; stage < 4; stage++) {
                    double km[4], dkm[4], kP[10], dkP[10];
                    cd_ekf4_tangent_stage(q, tm, tP, tdm, tdP, km, kP, dkm, dkP);
                    const double wgt = (stage == 0 || stage == 3) ? 1.0 : 2.0;
                    const double hdt = (stage == 2) ? dt : 0.5 * dt;
                    CGP_UNROLL for (int i = 0; i < 4; i++) {
                        am[i] = fma(wgt, km[i], am[i]); adm[i] = fma(wgt, dkm[i], adm[i]);
                        tm[i] = fma(hdt, km[i], m[i]); tdm[i] = fma(hdt, dkm[i], dm[i]);
                    }
                    CGP_UNROLL for (int i = 0; i < 10; i++) {
                        aP[i] = fma(wgt, kP[i], aP[i]); adP[i] = fma(wgt, dkP[i], adP[i]);
                        tP[i] = fma(hdt, kP[i], P[i]); tdP[i] = fma(hdt, dkP[i], dP[i]);
                    }
                }
                CGP_UNROLL for (int i = 0; i < 4; i++) { m[i] = fma(dt6, am[i], m[i]); dm[i] = fma(dt6, adm[i], dm[i]); }
                CGP_UNROLL for (int i = 0; i < 10; i++) { P[i] = fma(dt6, aP[i], P[i]); dP[i] = fma(dt6, adP[i], dP[i]); }
            }
            // ---- update and its tangent (the prediction is a copy: tangent_update reads it while it writes the state)
            double mp[4], dmp[4], Pp[10], dPp[10];
            CGP_UNROLL for (int i = 0; i < 4; i++) { mp[i] = m[i]; dmp[i] = dm[i]; }
            CGP_UNROLL for (int i = 0; i < 10; i++) { Pp[i] = P[i]; dPp[i] = dP[i]; }
            tangent_update<GAPS>(h, Xi, dXi, y, mp, dmp, Pp, dPp, m, dm, P, dP, nll, dnll);
        }
    }
    if (nll != nll) dnll = nll;                                           // a diverged filter: NaN in value and gradient
    if (dir == 0) io.nll[trial] = nll;
    io.grad[gi] = dnll;
}

hipError_t launch_cd_ekf4_tangent_substeps(const TangentIO& io, const ModelArgs& ma, bool gaps, hipStream_t stream) {
    if (io.B <= 0 || io.n_dir <= 0) return hipSuccess;
    const int64_t blocks = (io.B * io.n_dir + 63) / 64;
    if (gaps) hipLaunchKernelGGL((cd_ekf4_tangent_substeps_kernel<true>), dim3((unsigned)blocks), dim3(64), 0, stream, io, ma);
    else hipLaunchKernelGGL((cd_ekf4_tangent_substeps_kernel<false>), dim3((unsigned)blocks), dim3(64), 0, stream, io, ma);
    return hipGetLastError();
}
}  // namespace cgp
