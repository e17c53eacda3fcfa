// cgp_tangent4.hpp -- the EKF's negative log-likelihood AND its exact gradient in one launch (cgp_ekf_nll_grad): forward tangents of
// (m, P, nll) carried through the scan.
//
// The reference's drivers minimise obj(theta) = ekf(build_model(g(theta)), ys)[-1][-1] with value_and_grad THROUGH the scan
// (demos/ekfs_mle.py:43-51): an exact derivative.  Rounds 1 - 5 took central differences of 2 P + 1 filter passes (accurate to 1e-4 of
// the gradient).  Here one lane carries ONE tangent direction of one trial: the primal recursion of
// filters_smoothers.py:55-68, 222-264 on the chirp LCD model (models.py:264-311; SURVEY N1 for its Jacobian) and, beside it, the
// derivative of every quantity along the direction:
//     d mp = J dm + (d f)(m)                       d J = (dJ/dm)[dm] + (d J)            (d .) = the model's explicit dependence on the
//     d Pp = X + X^T + J dP J^T + d Sigma,  X = d J (J P)^T                              parameters along the direction
//     d S = h . d Pp h + d Xi      d K = (d Pp h - K d S) / S      d nu = -h . d mp
//     d mf = d mp + d K nu + K d nu        d Pf = d Pp - (d K K^T + K d K^T) S - K K^T d S
//     d nll += (d S / S + 2 nu d nu / S - nu^2 d S / S^2) / 2
// A direction is 24 doubles the HOST computes from the builder (chirpgp_amd/mle.py: complex-step derivatives of the model constants
// along theta_k): d log rho, d q, d M32_F (4), d M32_Sigma (3), d Xi, d m0 (4), d P0 (10, packed lower triangle).  The frequency
// state's chain (softplus, its first and second derivative, sin / cos) is differentiated in the kernel.  Nothing is approximated:
// the gradient agrees with the derivative taken in 100-digit arithmetic to rounding (tests/test_gpu_gradient.py: 1e-8).
//
// Layout: lane g = trial * n_dir + direction -- a trial's directions sit in neighbouring lanes and read the same measurements (one
// 64-byte request per eight steps, served once per trial by the cache).  Every lane repeats the primal (200 of its ~520 instructions a step):
// cheaper than exchanging it.  value = nll[trial] (written by direction 0), grad[trial][direction].
//
// The Fisher form (cgp_ekf_nll_fisher, kFisher): the same step, and from its two tangents d nu and d S the information of the Gaussian
// innovations model along the directions, F[i][j] = sum_t (d nu_i d nu_j / S + d S_i d S_j / (2 S^2)) -- the Gauss-Newton part of the
// NLL's Hessian.  Lane `dir` keeps row `dir` in registers and reads d nu_j, d S_j from lane base + j of its trial's group (ds_bpermute:
// no LDS memory, no barrier), so a trial must not straddle two wavefronts: 64 / n_dir whole trials per wavefront, the rest of the lanes
// idle.  F[i][j] and F[j][i] are the same instructions on commuted products: the matrix comes out exactly symmetric.
// The kernel is compiled for 4, 6, 8 and 16 row slots (kSlots >= n_dir; 6 is the chirp model's parameter count, cgp_inst_tangent4.hip).
// The source asks for a step's kSlots pairs of shuffles after the update (tangent_update hands back d nu and d S), unguarded, so that
// they and the update are one basic block; where they go is the compiler's scheduling.  In the gfx950 code of the 6-slot kernel all 24
// ds_bpermute stand in one run of 37 instructions at the END of the step, behind the covariance update (there too when the source asked
// for them between d nu and the gain), with the last operations of the NLL's increments between them; the row is then folded pair by
// pair under waits that count down (lgkmcnt 14, 12, .. 0) beside the tail of the mean's update.  So the layout buys one basic block
// and one stream of waits, not an overlap of the LDS round trip with the whole update.  (Guarded by j < n_dir one by one, every pair
// of shuffles was a basic block of its own with a wait of its own: 1.40 x the gradient kernel's time at six directions.)  Slots from
// n_dir on read some other lane and gather numbers nobody writes out.
#pragma once
#include "cgp_kernels.hpp"

namespace cgp {

constexpr int kDirDoubles = 24;      // d log rho | d q | d M (4) | d MS (3) | d Xi | d m0 (4) | d P0 (10)
constexpr int kFisherMaxDir = CGP_FISHER_MAX_DIR;      // a Fisher row lives in registers: 2 VGPRs per slot


// x of lane `src` of the wavefront (any lane: ds_bpermute on the two halves; the source lane must be active)
CGP_DEV double shuffle_f64(double x, int src) {
    const int lo = __builtin_amdgcn_ds_bpermute(src << 2, __double2loint(x));
    const int hi = __builtin_amdgcn_ds_bpermute(src << 2, __double2hiint(x));
    return __hiloint2double(hi, lo);
}

// The scalar update (filters_smoothers.py:55-68) with its tangent along one direction: from the predicted moments (mp, Pp) and their
// tangents to the filtered ones and the NLL's increments.  Symmetric matrices are packed lower triangles (00 10 11 20 21 22 30 31 32 33:
// Sym<4>::a).  The EKF kernel below calls it; the sigma-point kernel of cgp_tangent4_sigma.hpp spells the same expressions out, because
// through this function it compiled to fewer instructions and spills and yet measured 4 % slower (profiles/README.md).
struct TangentUpdate {
    double S, dS, iS, nu, dnu;           // the innovation, its variance and their tangents: what the Fisher forms take from a step
    // F[i][j] + d nu_i d nu_j / S + d S_i d S_j / (2 S^2) from this lane's (i) and another's (j) tangents: S is the trial's (the same bits
    // in all its lanes), and a product of two lanes' tangents is the same number in both of them
    CGP_DEV double fisher_add(double Fij, double nj, double sj) const {
        const double wn = iS, ws = 0.5 * iS * iS;
        return fma(dnu * nj, wn, fma(dS * sj, ws, Fij));
    }
};
// GAPS (CGP_SKIP_MISSING): a NaN measurement is a missing sample -- gate_missing (cgp_math.hpp) zeroes iS and nu, so that mf = mp, Pf = Pp,
// d mf = d mp, d Pf = d Pp, and the increments of d nll and of the Fisher row (weights iS, iS^2 / 2) are exact zeros; the NLL's own
// increment takes the third select.  No branch: a present measurement runs the operations of the unflagged step.  Defaulted: the
// unflagged kernels compile to what they compiled to.
template <bool GAPS = false>
CGP_DEV TangentUpdate tangent_update(const double (&h)[4], double Xi, double dXi, double y, const double (&mp)[4], const double (&dmp)[4],
                                     const double (&Pp)[10], const double (&dPp)[10], double (&m)[4], double (&dm)[4],
                                     double (&P)[10], double (&dP)[10], double& nll, double& dnll) {
    auto S_ = [](const double (&A)[10], int i, int j) { return A[Sym<4>::idx(i, j)]; };
    double PH[4], dPH[4];
    CGP_UNROLL for (int i = 0; i < 4; i++) {
        PH[i] = S_(Pp, i, 0) * h[0] + S_(Pp, i, 1) * h[1] + S_(Pp, i, 2) * h[2] + S_(Pp, i, 3) * h[3];
        dPH[i] = S_(dPp, i, 0) * h[0] + S_(dPp, i, 1) * h[1] + S_(dPp, i, 2) * h[2] + S_(dPp, i, 3) * h[3];
    }
    TangentUpdate u;
    u.S = h[0] * PH[0] + h[1] * PH[1] + h[2] * PH[2] + h[3] * PH[3] + Xi;
    u.dS = h[0] * dPH[0] + h[1] * dPH[1] + h[2] * dPH[2] + h[3] * dPH[3] + dXi;
    u.iS = rcp_nr(u.S);
    const double pred = h[0] * mp[0] + h[1] * mp[1] + h[2] * mp[2] + h[3] * mp[3];
    u.nu = y - pred;
    u.dnu = -(h[0] * dmp[0] + h[1] * dmp[1] + h[2] * dmp[2] + h[3] * dmp[3]);
    const bool gap = gate_missing<GAPS>(y, u.iS, u.nu);
    const double S = u.S, dS = u.dS, iS = u.iS, nu = u.nu, dnu = u.dnu;
    double K[4], dK[4];
    CGP_UNROLL for (int i = 0; i < 4; i++) { K[i] = PH[i] * iS; dK[i] = (dPH[i] - K[i] * dS) * iS; }
    CGP_UNROLL for (int i = 0; i < 4; i++) { m[i] = mp[i] + K[i] * nu; dm[i] = dmp[i] + dK[i] * nu + K[i] * dnu; }
    int kk = 0;
    CGP_UNROLL for (int i = 0; i < 4; i++) CGP_UNROLL for (int j = 0; j <= i; j++) {
        const double kk_ij = K[i] * K[j];
        P[kk] = Pp[kk] - kk_ij * S;
        dP[kk] = dPp[kk] - (dK[i] * K[j] + K[i] * dK[j]) * S - kk_ij * dS;
        kk++;
    }
    nll += gated_increment<GAPS>(gap, nll_increment(S, nu));
    dnll += 0.5 * (dS * iS + (2.0 * nu * dnu - nu * nu * dS * iS) * iS);
    return u;
}

// ---- the host side the tangent entry points share (cgp_inst_tangent4.hip, cgp_inst_tangent4_sgp.hip, cgp_inst_tangent4_cd.hip) is prepare_tangent with
// its TangentCall (cgp_args.hpp: the argument checks, the limit of the entry's own grid, io and ma filled); each entry then hands launch_on its launcher.

#ifndef CGP_TANGENT4_IO_ONLY      // the sigma-point units take TangentIO and not a second copy of this kernel
// GAPS: the update gated per lane on its trial's measurement (tangent_update; the lanes of a trial read the same y, the trials of a
// wavefront of the Fisher form need not) -- the shuffles stay unguarded.  Instantiated in cgp_inst_gaps4_tangent.hip only.
template <int kSlots, bool GAPS = false>      // 0: cgp_ekf_nll_grad; 4 / 6 / 8 / 16: cgp_ekf_nll_fisher with n_dir <= kSlots
__global__ void __launch_bounds__(64) ekf4_tangent_kernel(TangentIO io, ModelArgs ma) {
    constexpr bool kFisher = kSlots > 0;
    int64_t gidx;
    int base = 0;                                                         // kFisher: the first lane of this trial's group
    if constexpr (kFisher) {
        const int slot = (int)threadIdx.x / io.n_dir;                     // whole trials only: lanes from (64 / n_dir) n_dir on stay idle
        if (slot >= 64 / io.n_dir) return;
        base = slot * io.n_dir;
        const int64_t tr = (int64_t)blockIdx.x * (64 / io.n_dir) + slot;
        if (tr >= io.B) return;
        gidx = tr * io.n_dir + ((int)threadIdx.x - base);
    } else {
        gidx = (int64_t)blockIdx.x * 64 + threadIdx.x;
    }
    const int64_t total = io.B * io.n_dir;
    const bool active = gidx < total;
    if (!active) return;                                                  // (a partial wavefront runs with a partial EXEC mask)
    const int64_t gi = gidx;
    const int64_t trial = gi / io.n_dir;
    const int dir = (int)(gi - trial * io.n_dir);

    HarmonicLCD<1> model;
    model.setup(ma.params + trial * ma.param_stride, ma.dt, ma.model_id);
    const double rho = model.rho, q = model.q;
    const double M0 = model.M[0], M1 = model.M[1], M2 = model.M[2], M3 = model.M[3];
    const double scale = (kTwoPi * model.fs) * model.dt;                  // rotation angle = scale * softplus(u2)
    const double* __restrict__ dp = io.dirs + gi * kDirDoubles;
    const double dlr = dp[0], dq = dp[1], dM0 = dp[2], dM1 = dp[3], dM2 = dp[4], dM3 = dp[5];
    const double dS0 = dp[6], dS1 = dp[7], dS2 = dp[8], dXi = dp[9];
    double h[4];
    CGP_UNROLL for (int i = 0; i < 4; i++) h[i] = io.H[trial * io.H_stride + i];
    const double Xi = io.Xi[trial * io.Xi_stride];

    // state: m, P (packed lower triangle: 00 10 11 20 21 22 30 31 32 33) and their tangents
    double m[4], dm[4], P[10], dP[10];
    CGP_UNROLL for (int i = 0; i < 4; i++) { m[i] = io.m0[trial * io.m0_stride + i]; dm[i] = dp[10 + i]; }
    {
        const double* __restrict__ p0 = io.P0 + trial * io.P0_stride;
        int k = 0;
        CGP_UNROLL for (int i = 0; i < 4; i++) CGP_UNROLL for (int j = 0; j <= i; j++) { P[k] = p0[i * 4 + j]; dP[k] = dp[14 + k]; k++; }
    }
    double nll = 0.0, dnll = 0.0;
    double Frow[kFisher ? kSlots : 1];                                    // kFisher: row `dir` of F, constant indices only (registers)
    CGP_UNROLL for (int j = 0; j < (kFisher ? kSlots : 1); j++) Frow[j] = 0.0;
    (void)Frow;
    const double* __restrict__ rec = io.record(trial);
    auto S_ = [](const double (&A)[10], int i, int j) { return i >= j ? A[i * (i + 1) / 2 + j] : A[j * (j + 1) / 2 + i]; };

    for (int64_t t0 = 0; t0 < io.T; t0 += 8) {
        double yb[8];
        CGP_UNROLL for (int k = 0; k < 8; k++) yb[k] = (t0 + k < io.T) ? rec[t0 + k] : 0.0;
        const int n = (io.T - t0 < 8) ? (int)(io.T - t0) : 8;
        for (int k = 0; k < n; k++) {
            const double y = yb[k];
            // ---- the model at m: softplus and its two derivatives, the rotation
            double sp, dsp;
            softplus_pair(m[2], sp, dsp);
            const double th1 = scale * dsp;                               // d theta / d u2
            const double th2 = th1 * (1.0 - dsp);                         // d^2 theta / d u2^2   (sigmoid' = sigmoid (1 - sigmoid))
            double sn, cs;
            fast_sincos(scale * sp, sn, cs);
            const double rc = rho * cs, rs = rho * sn;
            const double mp0 = rc * m[0] - rs * m[1], mp1 = rs * m[0] + rc * m[1];
            const double mp2 = M0 * m[2] + M1 * m[3], mp3 = M2 * m[2] + M3 * m[3];
            const double J02 = -th1 * mp1, J12 = th1 * mp0;
            // ---- tangent of the model along the direction
            const double dth = th1 * dm[2], dth1 = th2 * dm[2];
            const double drc = dlr * rc - rs * dth, drs = dlr * rs + rc * dth;
            const double dmp0 = drc * m[0] - drs * m[1] + rc * dm[0] - rs * dm[1];
            const double dmp1 = drs * m[0] + drc * m[1] + rs * dm[0] + rc * dm[1];
            const double dmp2 = dM0 * m[2] + dM1 * m[3] + M0 * dm[2] + M1 * dm[3];
            const double dmp3 = dM2 * m[2] + dM3 * m[3] + M2 * dm[2] + M3 * dm[3];
            const double dJ02 = -(dth1 * mp1 + th1 * dmp1), dJ12 = dth1 * mp0 + th1 * dmp0;
            // ---- A = J P (rows of J: [rc, -rs, J02, 0], [rs, rc, J12, 0], [0, 0, M0, M1], [0, 0, M2, M3])
            double A[4][4], dA[4][4];      // dA = dJ P + J dP
            CGP_UNROLL for (int j = 0; j < 4; j++) {
                const double p0 = S_(P, 0, j), p1 = S_(P, 1, j), p2 = S_(P, 2, j), p3 = S_(P, 3, j);
                const double e0 = S_(dP, 0, j), e1 = S_(dP, 1, j), e2 = S_(dP, 2, j), e3 = S_(dP, 3, j);
                A[0][j] = rc * p0 - rs * p1 + J02 * p2;
                A[1][j] = rs * p0 + rc * p1 + J12 * p2;
                A[2][j] = M0 * p2 + M1 * p3;
                A[3][j] = M2 * p2 + M3 * p3;
                dA[0][j] = drc * p0 - drs * p1 + dJ02 * p2 + rc * e0 - rs * e1 + J02 * e2;
                dA[1][j] = drs * p0 + drc * p1 + dJ12 * p2 + rs * e0 + rc * e1 + J12 * e2;
                dA[2][j] = dM0 * p2 + dM1 * p3 + M0 * e2 + M1 * e3;
                dA[3][j] = dM2 * p2 + dM3 * p3 + M2 * e2 + M3 * e3;
            }
            // ---- Pp = A J^T + Sigma;  dPp = dA J^T + A dJ^T + dSigma   (lower triangle; column i of J^T = row i of J)
            double Pp[10], dPp[10];
            {
                int kk = 0;
                CGP_UNROLL for (int i = 0; i < 4; i++) CGP_UNROLL for (int j = 0; j <= i; j++) {
                    double v, dv;
                    if (j == 0) { v = A[i][0] * rc - A[i][1] * rs + A[i][2] * J02; dv = dA[i][0] * rc - dA[i][1] * rs + dA[i][2] * J02 + A[i][0] * drc - A[i][1] * drs + A[i][2] * dJ02; }
                    else if (j == 1) { v = A[i][0] * rs + A[i][1] * rc + A[i][2] * J12; dv = dA[i][0] * rs + dA[i][1] * rc + dA[i][2] * J12 + A[i][0] * drs + A[i][1] * drc + A[i][2] * dJ12; }
                    else if (j == 2) { v = A[i][2] * M0 + A[i][3] * M1; dv = dA[i][2] * M0 + dA[i][3] * M1 + A[i][2] * dM0 + A[i][3] * dM1; }
                    else { v = A[i][2] * M2 + A[i][3] * M3; dv = dA[i][2] * M2 + dA[i][3] * M3 + A[i][2] * dM2 + A[i][3] * dM3; }
                    Pp[kk] = v; dPp[kk] = dv; kk++;
                }
                Pp[0] += q; Pp[2] += q; Pp[5] += model.MS[0]; Pp[8] += model.MS[1]; Pp[9] += model.MS[2];          // Sigma = blockdiag(q, q, M32_Sigma)
                dPp[0] += dq; dPp[2] += dq; dPp[5] += dS0; dPp[8] += dS1; dPp[9] += dS2;
            }
            // ---- update and its tangent; kFisher: d nu and d S of the trial's other directions into this lane's row
            const double mpv[4] = {mp0, mp1, mp2, mp3}, dmpv[4] = {dmp0, dmp1, dmp2, dmp3};
            const TangentUpdate u = tangent_update<GAPS>(h, Xi, dXi, y, mpv, dmpv, Pp, dPp, m, dm, P, dP, nll, dnll);
            if constexpr (kFisher) {
                double nj[kSlots], sj[kSlots];
                CGP_UNROLL for (int j = 0; j < kSlots; j++) { nj[j] = shuffle_f64(u.dnu, base + j); sj[j] = shuffle_f64(u.dS, base + j); }
                CGP_UNROLL for (int j = 0; j < kSlots; j++) Frow[j] = u.fisher_add(Frow[j], nj[j], sj[j]);
            }
        }
    }
    if (active) {
        if constexpr (kFisher) {
            const bool diverged = nll != nll;                             // a diverged filter: NaN in all three outputs
            if (diverged) dnll = nll;
            double* __restrict__ row = io.fisher + gi * io.n_dir;
            CGP_UNROLL for (int j = 0; j < kSlots; j++) {
                if (j < io.n_dir) row[j] = diverged ? nll : Frow[j];
            }
        }
        if (dir == 0) io.nll[trial] = nll;
        io.grad[gi] = dnll;
    }
}

// kSlots > 0: 64 / n_dir whole trials per wavefront; 1 <= n_dir <= kSlots and ceil(B / (64 / n_dir)) < 2^31 (the caller).
template <int kSlots = 0, bool GAPS = false>
inline hipError_t launch_ekf4_tangent(const TangentIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.n_dir <= 0) return hipSuccess;                    // (T == 0 launches: the kernel skips its loop and writes nll = 0, grad = 0)
    const int64_t total = io.B * io.n_dir, tpw = 64 / io.n_dir;
    const int64_t blocks = kSlots > 0 ? (io.B + tpw - 1) / tpw : (total + 63) / 64;
    hipLaunchKernelGGL((ekf4_tangent_kernel<kSlots, GAPS>), dim3((unsigned)blocks), dim3(64), 0, stream, io, ma);
    return hipGetLastError();
}

// cgp_ekf_nll_fisher: the smallest compiled row that holds n_dir slots (a template: only the unit that calls it compiles its kernels)
template <bool GAPS = false>
inline hipError_t launch_ekf4_fisher(const TangentIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.n_dir <= 4) return launch_ekf4_tangent<4, GAPS>(io, ma, stream);
    if (io.n_dir <= 6) return launch_ekf4_tangent<6, GAPS>(io, ma, stream);
    if (io.n_dir <= 8) return launch_ekf4_tangent<8, GAPS>(io, ma, stream);
    return launch_ekf4_tangent<kFisherMaxDir, GAPS>(io, ma, stream);
}

#endif  // CGP_TANGENT4_IO_ONLY

// The GAPS instantiations (CGP_SKIP_MISSING) live in units of their own -- cgp_inst_gaps4_tangent.hip, cgp_inst_gaps4_tangent_sgp.hip -- so
// that the unflagged units compile to what they compiled to; fisher: the form that writes the matrix.
hipError_t launch_ekf4_tangent_gaps(const TangentIO& io, const ModelArgs& ma, bool fisher, hipStream_t stream);
hipError_t launch_sgp4_tangent_gaps(const TangentIO& io, const ModelArgs& ma, bool fisher, hipStream_t stream);
// The continuous-discrete sigma-point filter's tangent kernel (cgp_tangent4_cd_sigma.hpp) is reached through cgp_sgp_nll_grad: its two
// instantiations, cgp_inst_tangent4_cd_sgp.hip and cgp_inst_gaps4_tangent_cd_sgp.hip (CGP_RK4_SUBSTEPS is a trip count of either)
hipError_t launch_cd_sgp4_tangent_plain(const TangentIO& io, const ModelArgs& ma, hipStream_t stream);
hipError_t launch_cd_sgp4_tangent_gaps(const TangentIO& io, const ModelArgs& ma, hipStream_t stream);

}  // namespace cgp
