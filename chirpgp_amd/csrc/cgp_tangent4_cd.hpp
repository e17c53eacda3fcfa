// cgp_tangent4_cd.hpp -- the continuous-discrete EKF's negative log-likelihood AND its exact gradient in one launch (cgp_cd_ekf_nll_grad):
// forward tangents of (m, P, nll) carried through the four RK4 stages of the moment ODE and through the update.
//
// The reference fits the continuous-discrete models by value_and_grad of cd_ekf(...)[-1][-1] through the scan (demos/cd_ekfs_mle.py,
// tetralith/jobs/cd_ekfs_mle.py).  Per measurement cd_ekf takes one RK4 step (quadratures.py:34-54) of
//     dm/dt = a(m),      dP/dt = J P + P J^T + Gamma,      J = da/dm at m, Gamma = b b^T       (filters_smoothers.py:384-385)
// and then the scalar update (filters_smoothers.py:55-68).  On the d = 4 chirp / La Scala SDE (models.py:104-110; HarmonicSDE<1>):
//     w = 2 pi fs softplus(u2),   w' = 2 pi fs sigmoid(u2),   w'' = w' (1 - sigmoid(u2)),   gam = sqrt(3) / ell
//     a = [-lam u0 - w u1,  w u0 - lam u1,  u3,  -gam^2 u2 - 2 gam u3]
//     J = [-lam, -w, -w' u1, 0;   w, -lam, w' u0, 0;   0, 0, 0, 1;   0, 0, -gam^2, -2 gam]
// One lane carries ONE tangent direction of one trial, laid out as ekf4_tangent_kernel is (cgp_tangent4.hpp): lane g = trial * n_dir +
// direction, measurements in blocks of eight, nll[trial] written by direction 0, grad[trial][direction] by every lane.  Beside the primal
// every stage carries the derivative of its slopes along the direction (d . = the explicit dependence on the direction's constants):
//     d a  = J dm + (da/dlam) d lam + (da/dgam) d gam
//     d J  = (dJ/du2) dm2 + (dJ/du0, dJ/du1 through the w' column) + (dJ/dlam) d lam + (dJ/dgam) d gam
//     d (dP/dt) = (dJ P + J dP) + (dJ P + J dP)^T + d Gamma
// written ONCE (cd_ekf4_tangent_stage: (m, P, dm, dP) -> (k_m, k_P, dk_m, dk_P)) and called by a rolled loop over the four stages; the
// step length dt carries no tangent.  Then tangent_update<GAPS> of cgp_tangent4.hpp as it stands.  softplus and sigmoid are the accurate
// pair of the EKF tangent kernel (softplus_pair); the ODE's right-hand side has no sine or cosine.  Nothing is approximated.
//
// A direction is kCdDirDoubles = 27 doubles the HOST computes from the builder (chirpgp_amd/mle.py: tangent_directions_cd):
//     d lam | d gam | d Gamma (10, packed lower triangle) | d Xi | d m0 (4) | d P0 (10, packed lower triangle).
#pragma once
#include "cgp_tangent4.hpp"

namespace cgp {

constexpr int kCdDirDoubles = CGP_CD_DIR_DOUBLES;

// What a stage reads beside the state: the trial's constants and their tangents along this lane's direction
struct CdTangentModel {
    double lam, gam, fs, dlam, dgam;
    double G[10], dG[10];                // Gamma = b b^T and d Gamma, packed lower triangles
};

// The slopes of the moment ODE at (m, P) and their tangents along the direction (dm, dP).  Symmetric matrices are packed lower triangles
// (00 10 11 20 21 22 30 31 32 33), as in tangent_update.
CGP_DEV void cd_ekf4_tangent_stage(const CdTangentModel& q, const double (&m)[4], const double (&P)[10], const double (&dm)[4], const double (&dP)[10],
                                   double (&km)[4], double (&kP)[10], double (&dkm)[4], double (&dkP)[10]) {
    auto S_ = [](const double (&A)[10], int i, int j) { return i >= j ? A[i * (i + 1) / 2 + j] : A[j * (j + 1) / 2 + i]; };
    double sp, dsp;
    softplus_pair(m[2], sp, dsp);
    const double w = (kTwoPi * sp) * q.fs, w1 = (kTwoPi * dsp) * q.fs;    // w, dw / du2
    const double w2 = w1 * (1.0 - dsp);                                   // d^2 w / du2^2   (sigmoid' = sigmoid (1 - sigmoid))
    const double lam = q.lam, g2 = q.gam * q.gam, tg = 2.0 * q.gam;
    const double dlam = q.dlam, dg2 = tg * q.dgam, dtg = 2.0 * q.dgam;
    const double J02 = -w1 * m[1], J12 = w1 * m[0];
    // ---- tangent of the model along the direction
    const double dw = w1 * dm[2], dw1 = w2 * dm[2];
    const double dJ02 = -(dw1 * m[1] + w1 * dm[1]), dJ12 = dw1 * m[0] + w1 * dm[0];
    km[0] = -lam * m[0] - w * m[1];
    km[1] = w * m[0] - lam * m[1];
    km[2] = m[3];
    km[3] = -g2 * m[2] - tg * m[3];
    dkm[0] = -dlam * m[0] - dw * m[1] - lam * dm[0] - w * dm[1];
    dkm[1] = dw * m[0] - dlam * m[1] + w * dm[0] - lam * dm[1];
    dkm[2] = dm[3];
    dkm[3] = -dg2 * m[2] - dtg * m[3] - g2 * dm[2] - tg * dm[3];
    // ---- A = J P, dA = dJ P + J dP
    double A[4][4], dA[4][4];
    CGP_UNROLL for (int j = 0; j < 4; j++) {
        const double p0 = S_(P, 0, j), p1 = S_(P, 1, j), p2 = S_(P, 2, j), p3 = S_(P, 3, j);
        const double e0 = S_(dP, 0, j), e1 = S_(dP, 1, j), e2 = S_(dP, 2, j), e3 = S_(dP, 3, j);
        A[0][j] = -lam * p0 - w * p1 + J02 * p2;
        A[1][j] = w * p0 - lam * p1 + J12 * p2;
        A[2][j] = p3;
        A[3][j] = -g2 * p2 - tg * p3;
        dA[0][j] = -dlam * p0 - dw * p1 + dJ02 * p2 - lam * e0 - w * e1 + J02 * e2;
        dA[1][j] = dw * p0 - dlam * p1 + dJ12 * p2 + w * e0 - lam * e1 + J12 * e2;
        dA[2][j] = e3;
        dA[3][j] = -dg2 * p2 - dtg * p3 - g2 * e2 - tg * e3;
    }
    // ---- dP/dt = A + A^T + Gamma and its tangent (lower triangle)
    int kk = 0;
    CGP_UNROLL for (int i = 0; i < 4; i++) CGP_UNROLL for (int j = 0; j <= i; j++) {
        kP[kk] = (A[i][j] + A[j][i]) + q.G[kk];
        dkP[kk] = (dA[i][j] + dA[j][i]) + q.dG[kk];
        kk++;
    }
}

// GAPS: the update gated on the trial's measurement (tangent_update<true>); instantiated in cgp_inst_gaps4_tangent_cd.hip only.
template <bool GAPS>
__global__ void __launch_bounds__(64) cd_ekf4_tangent_kernel(TangentIO io, ModelArgs ma) {
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
    const double dt = ma.dt, dt6 = ma.dt / 6.0;
    double h[4];
    CGP_UNROLL for (int i = 0; i < 4; i++) h[i] = io.H[trial * io.H_stride + i];
    const double Xi = io.Xi[trial * io.Xi_stride];

    // state: m, P (packed lower triangle) and their tangents
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
            // ---- one RK4 step of (m, P) with its tangent (quadratures.py:49-54): x + dt (k1 + 2 k2 + 2 k3 + k4) / 6
            double tm[4], tdm[4], tP[10], tdP[10], am[4], adm[4], aP[10], adP[10];
            CGP_UNROLL for (int i = 0; i < 4; i++) { tm[i] = m[i]; tdm[i] = dm[i]; am[i] = 0.0; adm[i] = 0.0; }
            CGP_UNROLL for (int i = 0; i < 10; i++) { tP[i] = P[i]; tdP[i] = dP[i]; aP[i] = 0.0; adP[i] = 0.0; }
#pragma unroll 1
            for (int stage = 0; stage < 4; stage++) {
                double km[4], dkm[4], kP[10], dkP[10];
                cd_ekf4_tangent_stage(q, tm, tP, tdm, tdP, km, kP, dkm, dkP);
                const double wgt = (stage == 0 || stage == 3) ? 1.0 : 2.0;
                const double hdt = (stage == 2) ? dt : 0.5 * dt;           // the next stage's point: x + dt k / 2, the last one's x + dt k
                CGP_UNROLL for (int i = 0; i < 4; i++) {
                    am[i] = fma(wgt, km[i], am[i]); adm[i] = fma(wgt, dkm[i], adm[i]);
                    tm[i] = fma(hdt, km[i], m[i]); tdm[i] = fma(hdt, dkm[i], dm[i]);
                }
                CGP_UNROLL for (int i = 0; i < 10; i++) {
                    aP[i] = fma(wgt, kP[i], aP[i]); adP[i] = fma(wgt, dkP[i], adP[i]);
                    tP[i] = fma(hdt, kP[i], P[i]); tdP[i] = fma(hdt, dkP[i], dP[i]);
                }
            }
            double mp[4], dmp[4], Pp[10], dPp[10];
            CGP_UNROLL for (int i = 0; i < 4; i++) { mp[i] = fma(dt6, am[i], m[i]); dmp[i] = fma(dt6, adm[i], dm[i]); }
            CGP_UNROLL for (int i = 0; i < 10; i++) { Pp[i] = fma(dt6, aP[i], P[i]); dPp[i] = fma(dt6, adP[i], dP[i]); }
            // ---- update and its tangent
            tangent_update<GAPS>(h, Xi, dXi, y, mp, dmp, Pp, dPp, m, dm, P, dP, nll, dnll);
        }
    }
    if (nll != nll) dnll = nll;                                           // a diverged filter: NaN in value and gradient
    if (dir == 0) io.nll[trial] = nll;
    io.grad[gi] = dnll;
}

// 1 <= n_dir and ceil(B n_dir / 64) < 2^31 (the caller).  T == 0 launches: the kernel skips its loop and writes nll = 0, grad = 0.
template <bool GAPS>
inline hipError_t launch_cd_ekf4_tangent(const TangentIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.n_dir <= 0) return hipSuccess;
    const int64_t blocks = (io.B * io.n_dir + 63) / 64;
    hipLaunchKernelGGL((cd_ekf4_tangent_kernel<GAPS>), dim3((unsigned)blocks), dim3(64), 0, stream, io, ma);
    return hipGetLastError();
}

// The GAPS instantiation (CGP_SKIP_MISSING) lives in a unit of its own, cgp_inst_gaps4_tangent_cd.hip, as the other tangent kernels' do.
hipError_t launch_cd_ekf4_tangent_gaps(const TangentIO& io, const ModelArgs& ma, hipStream_t stream);
// CGP_RK4_SUBSTEPS: a kernel template of its own, cd_ekf4_tangent_substeps_kernel<GAPS> in cgp_inst_substeps4_tangent_cd.hip -- the kernel
// above with its four-stage loop run n = ma.substeps times per sample, on the stage function above.  The two stay two texts: with the RK4
// step in one function of both, the plain form's gradient moves in its last bits on the MI355X (profiles/tangent_sharing_trial.txt).
hipError_t launch_cd_ekf4_tangent_substeps(const TangentIO& io, const ModelArgs& ma, bool gaps, hipStream_t stream);

}  // namespace cgp
