// cgp_tangent4_sigma.hpp -- the sigma-point filter's negative log-likelihood AND its exact gradient in one launch (cgp_sgp_nll_grad):
// forward tangents of (m, P, nll) carried through the scan of sgp_filter (filters_smoothers.py:446-490, prediction :88-121) on the
// d = 4 chirp / La Scala LCD models, for ANY d = 4 sigma-point set (Gauss-Hermite, cubature, unscented: the literal per-point sums).
//
// The reference's GHFS drivers minimise sgp_filter(build_model(g(theta)), ys)[-1][-1] with value_and_grad THROUGH the scan
// (demos/ghfs_mle.py:53-56).  Along one direction (the 24 model-constant derivatives of cgp_tangent4.hpp, CGP_DIR_DOUBLES) a step is
//     P = L L^T                      dL = L Phi(L^-1 dP L^-T)   (Phi: strict lower triangle + half the diagonal), taken column by column:
//                                    dL_jj = (dP_jj - 2 sum_k<j L_jk dL_jk) / (2 L_jj),
//                                    dL_ij = (dP_ij - sum_k<j (dL_ik L_jk + L_ik dL_jk) - L_ij dL_jj) / L_jj
//     chi_p = m + L xi_p             d chi_p = dm + dL xi_p
//     f_p = blockdiag(rho Rot(theta(chi_p,2)), M) chi_p        d f_p = J(chi_p) d chi_p + (d f)(chi_p)   (the EKF tangent's partials at chi_p)
//     mp = sum w f                   d mp = sum w d f
//     Pp = sum w f f^T + (sum w) Sigma - mp mp^T               d Pp = sum w (d f f^T + f d f^T) + (sum w) d Sigma - d mp mp^T - mp d mp^T
// and the scalar update with its tangent exactly as cgp_tangent4.hpp (tangent_update).  Nothing is approximated.
//
// Layout: one wavefront per trial (block = trial).
//   * The primal state (m, P) and the update are replicated in every lane, as in the cooperative filter's fan (cgp_coop4_sigma.hpp).
//   * Lane k < nd OWNS direction k: its (dm, dP) live in that lane's registers, and the lane differentiates the Cholesky factor and the
//     update for its direction alone -- the per-direction work runs across lanes instead of being repeated in every one.
//   * The fan runs one sigma point per lane (p = lane, lane + 64, ...), reading (dm, dL, d log rho, d M) of the directions from a small LDS
//     table (broadcast reads) the owners fill.  It runs in passes of 28 partial sums -- the primal's 14 and direction 0's, then two
//     directions at a time -- each reduced in one call of the fan's LDS reduction (coop_reduce_to_lds), rather than keeping 14
//     accumulators per direction live (256 VGPRs and scratch from six directions on).  The lane's points are evaluated in pass 0 and
//     kept (sets of up to 128 points; larger ones are re-evaluated in every pass).
// Up to kSgpMaxDir directions per launch; more run as slices, one launch each.  A failed Cholesky poisons L and with it every sum: nll
// and grad are NaN, as sgp_filter writes.  T == 0 writes nll = 0, grad = 0.
//
// The Fisher form (cgp_sgp_nll_fisher, kFisher): owner k also keeps row k of F[i][j] = sum_t (d nu_i d nu_j / S + d S_i d S_j / (2 S^2))
// in registers; the source lane j is uniform, so d nu_j and d S_j come by v_readlane.  F couples all the directions of a launch: no
// slices, n_dir <= kSgpMaxDir.
#pragma once
#include "cgp_coop4_sigma.hpp"
#include "cgp_tangent4.hpp"

namespace cgp {

constexpr int kSgpMaxDir = 16;           // directions per launch (the lanes that own one)
constexpr int kSgpDirPitch = 20;         // LDS per direction: d m (4) | d L (10, packed lower triangle) | d log rho | d M (4) | pad
constexpr int kSgpSums = 14;             // partial sums per primal / direction: mean (4) + second moment (10, packed)

struct SgpTangentIO {
    TangentIO t;                         // records, initial condition, dirs [B][n_dir][24], nll [B], grad [B][n_dir]
    int dir0, nd;                        // this launch's slice of directions: dir0 .. dir0 + nd - 1
};

// One sigma point of the fan: its primal evaluation (chi, f = the model's mean at chi, the rotation and d theta / d chi_2) and the partial
// sums it contributes.  A point beyond the set (p >= s) gets weight 0 and xi = 0: it adds exact zeros.
struct FanPoint {
    double xi[4], w, chi[4], f[4], wf[4], rc, rs, th1;
    CGP_DEV void eval(const SigmaSet& sg, int p, int s, const double (&m)[4], const Sym<4>& L, double rho, double scale,
                      double M0, double M1, double M2, double M3) {
        const bool valid = p < s;
        const int pc = valid ? p : 0;
        CGP_UNROLL for (int j = 0; j < 4; j++) xi[j] = valid ? sg.template coord<true>(pc * 4 + j) : 0.0;
        w = valid ? sg.template weight<true>(pc) : 0.0;
        CGP_UNROLL for (int i = 0; i < 4; i++) {
            double t = L(i, 0) * xi[0];
            CGP_UNROLL for (int j = 1; j <= i; j++) t = fma(L(i, j), xi[j], t);
            chi[i] = m[i] + t;
        }
        double sp, dsp;
        softplus_pair(chi[2], sp, dsp);
        th1 = scale * dsp;                                                // d theta / d chi_2
        double sn, cs;
        fast_sincos(scale * sp, sn, cs);
        rc = rho * cs; rs = rho * sn;
        f[0] = rc * chi[0] - rs * chi[1]; f[1] = rs * chi[0] + rc * chi[1];
        f[2] = M0 * chi[2] + M1 * chi[3]; f[3] = M2 * chi[2] + M3 * chi[3];
        CGP_UNROLL for (int i = 0; i < 4; i++) wf[i] = w * f[i];
    }
    // w f, w f f^T
    CGP_DEV void add_primal(double* a) const {
        CGP_UNROLL for (int i = 0; i < 4; i++) a[i] += wf[i];
        CGP_UNROLL for (int i = 0; i < 4; i++)
            CGP_UNROLL for (int j = 0; j <= i; j++) a[4 + Sym<4>::idx(i, j)] = fma(wf[i], f[j], a[4 + Sym<4>::idx(i, j)]);
    }
    // w df, w (df f^T + f df^T) along the direction stored at e (LDS): df = J(chi) d chi + (d f)(chi), d chi = dm + dL xi
    CGP_DEV void add_tangent(const double* e, double* a, double M0, double M1, double M2, double M3) const {
        double dchi[4];
        CGP_UNROLL for (int i = 0; i < 4; i++) {
            double t = e[i];
            CGP_UNROLL for (int j = 0; j <= i; j++) t = fma(e[4 + Sym<4>::idx(i, j)], xi[j], t);
            dchi[i] = t;
        }
        const double elr = e[14], eM0 = e[15], eM1 = e[16], eM2 = e[17], eM3 = e[18];
        const double dth = th1 * dchi[2];
        const double drc = elr * rc - rs * dth, drs = elr * rs + rc * dth;
        const double df[4] = {drc * chi[0] - drs * chi[1] + rc * dchi[0] - rs * dchi[1],
                              drs * chi[0] + drc * chi[1] + rs * dchi[0] + rc * dchi[1],
                              eM0 * chi[2] + eM1 * chi[3] + M0 * dchi[2] + M1 * dchi[3],
                              eM2 * chi[2] + eM3 * chi[3] + M2 * dchi[2] + M3 * dchi[3]};
        double wdf[4];
        CGP_UNROLL for (int i = 0; i < 4; i++) { wdf[i] = w * df[i]; a[i] += wdf[i]; }
        CGP_UNROLL for (int i = 0; i < 4; i++)
            CGP_UNROLL for (int j = 0; j <= i; j++)
                a[4 + Sym<4>::idx(i, j)] = fma(wdf[i], f[j], fma(wf[i], df[j], a[4 + Sym<4>::idx(i, j)]));
    }
};

// GAPS (CGP_SKIP_MISSING): the update gated on the step's measurement, the wavefront's one y (gate_missing, cgp_math.hpp; as tangent_update
// of cgp_tangent4.hpp).  Instantiated in cgp_inst_gaps4_tangent_sgp.hip only.
template <bool kFisher, bool GAPS = false>
__global__ void __launch_bounds__(64) sgp4_tangent_kernel(SgpTangentIO sio, ModelArgs ma) {
    __shared__ double red[kFanLdsDoubles];
    __shared__ __attribute__((aligned(16))) double dtab[(kSgpMaxDir + 1) * kSgpDirPitch];
    const TangentIO& io = sio.t;
    const int lane = threadIdx.x;
    const int64_t trial = blockIdx.x;
    if (trial >= io.B) return;

    HarmonicLCD<1> model;
    model.setup(ma.params + trial * ma.param_stride, ma.dt, ma.model_id);
    const double rho = model.rho;
    const double M0 = model.M[0], M1 = model.M[1], M2 = model.M[2], M3 = model.M[3];
    const double scale = (kTwoPi * model.fs) * model.dt;                  // rotation angle = scale * softplus(chi_2)
    SigmaSet sg = ma.sg;
    sg.stage(dyn_lds(), lane, 64, 4);
    const int s = sg.s;
    double wsum = 0.0;                                                    // sum w: Pp = sum w (f f^T + Sigma) - mp mp^T
    for (int p = 0; p < s; p++) wsum += sg.template weight<true>(p);
    Sym<4> Sig;                                                           // blockdiag(q, q, M32_Sigma)
    CGP_UNROLL for (int k = 0; k < Sym<4>::N; k++) Sig.a[k] = 0.0;
    model.add_sigma(Sig, 1.0);

    // ---- this lane's direction (lanes from nd on carry a zero direction and write nothing)
    const int nd = sio.nd;
    const bool owner = lane < nd;
    const int my_pass = (lane + 1) / 2, my_slot = (lane & 1) ? 0 : kSgpSums;   // where this direction's sums come out (see the fan)
    double dlr = 0.0, dq = 0.0, dM[4] = {0.0, 0.0, 0.0, 0.0}, dS[3] = {0.0, 0.0, 0.0}, dXi = 0.0;
    double dm[4] = {0.0, 0.0, 0.0, 0.0};
    Sym<4> dP;
    CGP_UNROLL for (int k = 0; k < Sym<4>::N; k++) dP.a[k] = 0.0;
    if (owner) {
        const double* __restrict__ dp = io.dirs + (trial * io.n_dir + sio.dir0 + lane) * kDirDoubles;
        dlr = dp[0]; dq = dp[1];
        CGP_UNROLL for (int i = 0; i < 4; i++) dM[i] = dp[2 + i];
        CGP_UNROLL for (int i = 0; i < 3; i++) dS[i] = dp[6 + i];
        dXi = dp[9];
        CGP_UNROLL for (int i = 0; i < 4; i++) dm[i] = dp[10 + i];
        CGP_UNROLL for (int k = 0; k < Sym<4>::N; k++) dP.a[k] = dp[14 + k];
    }
    const bool writer = lane <= kSgpMaxDir;                               // rows nd .. kSgpMaxDir stay zero
    if (writer) {
        double* e = dtab + lane * kSgpDirPitch;
        e[14] = dlr;
        CGP_UNROLL for (int i = 0; i < 4; i++) e[15 + i] = dM[i];
    }
    Sym<4> dSig;
    CGP_UNROLL for (int k = 0; k < Sym<4>::N; k++) dSig.a[k] = 0.0;
    dSig(0, 0) = dq; dSig(1, 1) = dq; dSig(2, 2) = dS[0]; dSig(3, 2) = dS[1]; dSig(3, 3) = dS[2];

    double h[4];
    CGP_UNROLL for (int i = 0; i < 4; i++) h[i] = io.H[trial * io.H_stride + i];
    const double Xi = io.Xi[trial * io.Xi_stride];
    double m[4];
    CGP_UNROLL for (int i = 0; i < 4; i++) m[i] = io.m0[trial * io.m0_stride + i];
    Sym<4> P;
    {
        const double* __restrict__ p0 = io.P0 + trial * io.P0_stride;
        CGP_UNROLL for (int i = 0; i < 4; i++) CGP_UNROLL for (int j = 0; j <= i; j++) P(i, j) = p0[i * 4 + j];
    }
    double nll = 0.0, dnll = 0.0;
    double Frow[kFisher ? kFisherMaxDir : 1];                             // kFisher: row `lane` of F, constant indices only (registers)
    CGP_UNROLL for (int j = 0; j < (kFisher ? kFisherMaxDir : 1); j++) Frow[j] = 0.0;
    (void)Frow;
    const double* __restrict__ ys = io.record(trial);
    const int64_t T = io.T;
    const bool narrow = s <= 32;                                          // only lanes 0..31 hold points: half the reduction work
    // The fan runs in passes of two slots of kSgpSums sums each -- one LDS reduction of 28 values per pass, 28 accumulators per lane:
    //     pass 0: slot A = the primal sums (w f, w f f^T), slot B = direction 0;   pass k >= 1: directions 2 k - 1 (A) and 2 k (B)
    // (a direction's sums are w df, w (df f^T + f df^T)).  A pass re-evaluates the lane's points (chi, softplus, sin / cos): cheaper than
    // keeping nd x 14 accumulators live.
    const int npass = 1 + nd / 2;

    for (int64_t t0 = 0; t0 < T; t0 += 64) {
        const double ychunk = (t0 + lane < T) ? ys[t0 + lane] : 0.0;
        const int nsteps = (T - t0 < 64) ? (int)(T - t0) : 64;
        for (int k = 0; k < nsteps; k++) {
            const double y = readlane_f64(ychunk, k);
            // ---- Cholesky factor (replicated) and its tangent along this lane's direction
            Sym<4> L, dL;
            Vec<4> inv;
            cholesky<4>(P, L, inv);
            CGP_UNROLL for (int j = 0; j < 4; j++) {
                double sd = dP(j, j);
                CGP_UNROLL for (int c = 0; c < j; c++) sd = fma(-2.0 * L(j, c), dL(j, c), sd);
                dL(j, j) = 0.5 * sd * inv.v[j];
                CGP_UNROLL for (int i = j + 1; i < 4; i++) {
                    double t = dP(i, j);
                    CGP_UNROLL for (int c = 0; c < j; c++) t = fma(-dL(i, c), L(j, c), fma(-L(i, c), dL(j, c), t));
                    dL(i, j) = fma(-L(i, j), dL(j, j), t) * inv.v[j];
                }
            }
            if (writer) {
                double* e = dtab + lane * kSgpDirPitch;
                CGP_UNROLL for (int i = 0; i < 4; i++) e[i] = owner ? dm[i] : 0.0;
                CGP_UNROLL for (int c = 0; c < Sym<4>::N; c++) e[4 + c] = owner ? dL.a[c] : 0.0;
            }
            wave_lds_fence();
            // ---- the fan, pass by pass; each lane keeps the totals it needs: the primal ones and its own direction's.  A lane takes its
            // points two at a time (p = base + lane and base + lane + 64: two independent chains in one basic block), and with at most
            // 128 points it evaluates them once per step, in pass 0, and keeps them for the later passes.
            double tp[kSgpSums], td[kSgpSums];
            FanPoint pt[2];
#pragma unroll 1
            for (int pass = 0; pass < npass; pass++) {
                const bool first = pass == 0;
                const double* eA = dtab + (first ? 0 : 2 * pass - 1) * kSgpDirPitch;
                const double* eB = dtab + 2 * pass * kSgpDirPitch;
                double acc[2 * kSgpSums];
                CGP_UNROLL for (int c = 0; c < 2 * kSgpSums; c++) acc[c] = 0.0;
                for (int base = 0; base < s; base += 128) {
                    if (first || s > 128) {
                        CGP_UNROLL for (int q = 0; q < 2; q++) pt[q].eval(sg, base + lane + 64 * q, s, m, L, rho, scale, M0, M1, M2, M3);
                    }
                    CGP_UNROLL for (int q = 0; q < 2; q++) {
                        if (first) pt[q].add_primal(acc); else pt[q].add_tangent(eA, acc, M0, M1, M2, M3);
                    }
                    CGP_UNROLL for (int q = 0; q < 2; q++) pt[q].add_tangent(eB, acc + kSgpSums, M0, M1, M2, M3);
                }
                const double* tot = coop_reduce_to_lds<2 * kSgpSums>(acc, red, lane, narrow);
                if (first) CGP_UNROLL for (int c = 0; c < kSgpSums; c++) tp[c] = tot[c];
                const bool mine = pass == my_pass;
                CGP_UNROLL for (int c = 0; c < kSgpSums; c++) { const double v = tot[my_slot + c]; td[c] = mine ? v : td[c]; }
                wave_lds_fence();
            }
            // ---- predicted moments (replicated) and this lane's direction's tangents of them
            const double mp[4] = {tp[0], tp[1], tp[2], tp[3]};
            double dmp[4];
            CGP_UNROLL for (int i = 0; i < 4; i++) dmp[i] = td[i];
            Sym<4> Pp, dPp;
            CGP_UNROLL for (int i = 0; i < 4; i++)
                CGP_UNROLL for (int j = 0; j <= i; j++) {
                    const int c = Sym<4>::idx(i, j);
                    Pp.a[c] = fma(wsum, Sig.a[c], tp[4 + c]) - mp[i] * mp[j];
                    dPp.a[c] = fma(wsum, dSig.a[c], td[4 + c]) - (dmp[i] * mp[j] + mp[i] * dmp[j]);
                }
            // ---- update (filters_smoothers.py:55-68) and its tangent, spelled out: through tangent_update of cgp_tangent4.hpp (the same expressions, the EKF
            // kernel's copy) cgp_sgp_nll_fisher measured 4 % slower on the MI355X, with fewer instructions and spills (profiles/README.md)
            double PH[4], dPH[4];
            CGP_UNROLL for (int i = 0; i < 4; i++) {
                PH[i] = Pp(i, 0) * h[0] + Pp(i, 1) * h[1] + Pp(i, 2) * h[2] + Pp(i, 3) * h[3];
                dPH[i] = dPp(i, 0) * h[0] + dPp(i, 1) * h[1] + dPp(i, 2) * h[2] + dPp(i, 3) * h[3];
            }
            const double S = h[0] * PH[0] + h[1] * PH[1] + h[2] * PH[2] + h[3] * PH[3] + Xi;
            const double dS_ = h[0] * dPH[0] + h[1] * dPH[1] + h[2] * dPH[2] + h[3] * dPH[3] + dXi;
            double iS = rcp_nr(S);
            const double pred = h[0] * mp[0] + h[1] * mp[1] + h[2] * mp[2] + h[3] * mp[3];
            double nu = y - pred;
            const double dnu = -(h[0] * dmp[0] + h[1] * dmp[1] + h[2] * dmp[2] + h[3] * dmp[3]);
            const bool gap = gate_missing<GAPS>(y, iS, nu);                // GAPS and a NaN y: iS = nu = 0; otherwise nothing, false
            double K[4], dK[4];
            CGP_UNROLL for (int i = 0; i < 4; i++) { K[i] = PH[i] * iS; dK[i] = (dPH[i] - K[i] * dS_) * iS; }
            CGP_UNROLL for (int i = 0; i < 4; i++) { m[i] = mp[i] + K[i] * nu; dm[i] = dmp[i] + dK[i] * nu + K[i] * dnu; }
            CGP_UNROLL for (int i = 0; i < 4; i++)
                CGP_UNROLL for (int j = 0; j <= i; j++) {
                    const double kk = K[i] * K[j];
                    P(i, j) = Pp(i, j) - kk * S;
                    dP(i, j) = dPp(i, j) - (dK[i] * K[j] + K[i] * dK[j]) * S - kk * dS_;
                }
            nll += gated_increment<GAPS>(gap, nll_increment(S, nu));
            dnll += 0.5 * (dS_ * iS + (2.0 * nu * dnu - nu * nu * dS_ * iS) * iS);
            if constexpr (kFisher) {
                // F[lane][j] += d nu_lane d nu_j / S + d S_lane d S_j / (2 S^2), as cgp_tangent4.hpp: S is replicated, the products commute
                const double wn = iS, ws = 0.5 * iS * iS;
                CGP_UNROLL for (int j = 0; j < kFisherMaxDir; j++) {
                    if (j < nd) {                                         // (uniform)
                        const double nj = readlane_f64(dnu, j), sj = readlane_f64(dS_, j);
                        Frow[j] = fma(dnu * nj, wn, fma(dS_ * sj, ws, Frow[j]));
                    }
                }
            }
        }
    }
    // (T == 0: nll = 0, grad = 0, fisher = 0)
    if constexpr (kFisher) {
        const bool diverged = nll != nll;                                 // a Cholesky that broke down: NaN in all three outputs
        if (diverged) dnll = nll;
        if (owner) {
            double* __restrict__ row = io.fisher + (trial * io.n_dir + lane) * io.n_dir;      // (one launch: dir0 = 0, nd = n_dir)
            CGP_UNROLL for (int j = 0; j < kFisherMaxDir; j++) {
                if (j < nd) row[j] = diverged ? nll : Frow[j];
            }
        }
    }
    if (lane == 0 && sio.dir0 == 0) io.nll[trial] = nll;
    if (owner) io.grad[trial * io.n_dir + sio.dir0 + lane] = dnll;
}

// One launch per slice of kSgpMaxDir directions; every slice repeats the primal (nll is written by the first).  B < 2^31 (the caller).
// kKernel: an instantiation of sgp4_tangent_kernel or of cd_sgp4_tangent_kernel (cgp_tangent4_cd_sigma.hpp).
template <void (*kKernel)(SgpTangentIO, ModelArgs)>
inline hipError_t launch_tangent_slices(const TangentIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.n_dir <= 0) return hipSuccess;
    for (int dir0 = 0; dir0 < io.n_dir; dir0 += kSgpMaxDir) {
        SgpTangentIO sio;
        sio.t = io; sio.dir0 = dir0;
        sio.nd = io.n_dir - dir0 < kSgpMaxDir ? io.n_dir - dir0 : kSgpMaxDir;
        hipLaunchKernelGGL(kKernel, dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, sio, ma);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// kFisher: n_dir <= kSgpMaxDir (the caller), so there is one slice with every direction in it.
template <bool kFisher = false, bool GAPS = false>
inline hipError_t launch_sgp4_tangent(const TangentIO& io, const ModelArgs& ma, hipStream_t stream) {
    return launch_tangent_slices<sgp4_tangent_kernel<kFisher, GAPS>>(io, ma, stream);
}

}  // namespace cgp
