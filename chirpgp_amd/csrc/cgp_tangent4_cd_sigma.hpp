// cgp_tangent4_cd_sigma.hpp -- the continuous-discrete sigma-point filter's negative log-likelihood AND its exact gradient in one launch
// (cgp_sgp_nll_grad with a CGP_M_HARMONIC_SDE model): forward tangents of (m, P, nll) carried through the four RK4 stages of the
// sigma-point moment ODE of cd_sgp_filter (filters_smoothers.py:534-582, the right-hand side :124-137) and through the update, on the
// d = 4 chirp / La Scala SDE, for ANY d = 4 sigma-point set (the literal per-point sums).
//
// The reference's GHFS drivers of the continuous-discrete models minimise cd_sgp_filter(...)[-1][-1] with value_and_grad THROUGH the
// scan (demos/cd_ghfs_mle.py).  Per measurement the filter takes one RK4 step (quadratures.py:34-54) of
//     P = L L^T,   chi_p = m + L xi_p,   dm/dt = sum w_p a(chi_p),   dP/dt = C + C^T + Gamma,   C = sum w_p (chi_p - m) a(chi_p)^T
// with the drift of the SDE (models.py:104-110; HarmonicSDE<1>)
//     w = 2 pi fs softplus(u2),   w' = 2 pi fs sigmoid(u2),   gam = sqrt(3) / ell
//     a(u) = [-lam u0 - w u1,  w u0 - lam u1,  u3,  -gam^2 u2 - 2 gam u3]
// and then the scalar update (filters_smoothers.py:55-68).  Along one direction (the 27 constants of cgp_tangent4_cd.hpp,
// CGP_CD_DIR_DOUBLES) a stage is
//     dL = L Phi(L^-1 dP L^-T)       column by column, the lines of cgp_tangent4_sigma.hpp a second time (see the layout below)
//     d chi_p = dm + dL xi_p         d (chi_p - m) = dL xi_p
//     d a_p = J(chi_p) d chi_p + (da/dlam) d lam + (da/dgam) d gam       (the drift has no sine or cosine, and its tangent needs no
//                                                                         second derivative of softplus)
//     d (dm/dt) = sum w_p d a_p      d (dP/dt) = dC + dC^T + d Gamma,    dC = sum w_p (dL xi_p a_p^T + L xi_p d a_p^T)
// written ONCE (cd_sgp4_tangent_stage below) and called by a rolled loop over the four stages, n = CGP_RK4_SUBSTEPS times per sample at
// h = dt / n (a run-time trip count: n = 1 is the plain call); the step length carries no tangent.  Nothing is approximated.
//
// Layout: that of sgp4_tangent_kernel (cgp_tangent4_sigma.hpp) -- one wavefront per trial, the primal replicated in every lane, lane
// k < nd OWNS direction k, the fan one sigma point per lane in 1 + nd / 2 passes of 28 partial sums, each reduced by coop_reduce_to_lds;
// up to kSgpMaxDir directions per launch, more as slices (launch_tangent_slices of that header).  The Cholesky tangent and the fan's pass
// loop are that kernel's lines a second time in the stage below, not functions of both: shared, they change sgp4_tangent_kernel's bits
// or make it 4 % slower (profiles/tangent_sharing_trial.txt).  What is new is where the RK4 step's state lives.  Base point, stage point and
// accumulators are 3 x 14 doubles of primal and 3 x 14 of tangent; the fan (sgp4_tangent_kernel: 396 of the 512 VGPRs) reads none of
// them but the stage point, and that only through L and the direction table.  So across the fan the base point and the accumulators
// are PARKED in LDS: the replicated primal once per wavefront (lane 0 writes, every lane reads the same address back), the tangents in a
// row per owner lane.  A stage reads its point from registers, factorises, fans, and then combines against the parked rows.
//
// A Cholesky that breaks down at any stage poisons L and with it every sum of that stage and all that follows: nll and grad are NaN, as
// cd_sgp_filter writes.  T == 0 writes nll = 0, grad = 0.
#pragma once
#include "cgp_tangent4_sigma.hpp"
#include "cgp_tangent4_cd.hpp"

namespace cgp {

constexpr int kCdSgpDirDoubles = 16;     // of the direction table's pitch of kSgpDirPitch: d m (4) | d L (10) | d lam | d gam
constexpr int kCdSgpParkPitch = 30;      // a parked row: base point (m 4 | P 10) | accumulators (4 | 10) | pad (an odd number of 16-byte pairs)
constexpr int kCdSgpParkRows = 2 + kSgpMaxDir;      // row 0: the replicated primal; row 1 + k: owner lane k's tangents; the last: zeros, the other lanes'
static_assert(kCdSgpParkRows * kCdSgpParkPitch * sizeof(double) <= (size_t)kCdSgpParkBytes, "prepare_tangent leaves kCdSgpParkBytes of LDS to the parked rows");
static_assert(kCdSgpDirDoubles <= kSgpDirPitch, "the direction table's rows");

// One sigma point of the fan: chi = m + L xi, lx = L xi = chi - m, the drift a at chi and w' there.  A point beyond the set (p >= s) gets
// weight 0 and xi = 0: it adds exact zeros.
struct CdFanPoint {
    double xi[4], w, lx[4], chi[4], a[4], wa[4], om, om1;
    CGP_DEV void eval(const SigmaSet& sg, int p, int s, const double (&m)[4], const Sym<4>& L, double lam, double g2, double tg, double fs) {
        const bool valid = p < s;
        const int pc = valid ? p : 0;
        CGP_UNROLL for (int j = 0; j < 4; j++) xi[j] = valid ? sg.template coord<true>(pc * 4 + j) : 0.0;
        w = valid ? sg.template weight<true>(pc) : 0.0;
        CGP_UNROLL for (int i = 0; i < 4; i++) {
            double t = L(i, 0) * xi[0];
            CGP_UNROLL for (int j = 1; j <= i; j++) t = fma(L(i, j), xi[j], t);
            lx[i] = t;
            chi[i] = m[i] + t;
        }
        double sp, dsp;
        softplus_pair(chi[2], sp, dsp);
        om = (kTwoPi * sp) * fs; om1 = (kTwoPi * dsp) * fs;                                  // w(chi_2) and dw / d chi_2
        a[0] = -lam * chi[0] - om * chi[1];
        a[1] = om * chi[0] - lam * chi[1];
        a[2] = chi[3];
        a[3] = -g2 * chi[2] - tg * chi[3];
        CGP_UNROLL for (int i = 0; i < 4; i++) wa[i] = w * a[i];
    }
    // w a, w (lx a^T + a lx^T)
    CGP_DEV void add_primal(double* acc) const {
        CGP_UNROLL for (int i = 0; i < 4; i++) acc[i] += wa[i];
        CGP_UNROLL for (int i = 0; i < 4; i++)
            CGP_UNROLL for (int j = 0; j <= i; j++) acc[4 + Sym<4>::idx(i, j)] = fma(lx[i], wa[j], fma(lx[j], wa[i], acc[4 + Sym<4>::idx(i, j)]));
    }
    // w da, w (dlx a^T + lx da^T + sym.) along the direction stored at e (LDS): d chi = dm + dL xi, dlx = dL xi
    CGP_DEV void add_tangent(const double* e, double* acc, double lam, double g2, double tg) const {
        double dlx[4], dchi[4];
        CGP_UNROLL for (int i = 0; i < 4; i++) {
            double t = e[4 + Sym<4>::idx(i, 0)] * xi[0];
            CGP_UNROLL for (int j = 1; j <= i; j++) t = fma(e[4 + Sym<4>::idx(i, j)], xi[j], t);
            dlx[i] = t;
            dchi[i] = e[i] + t;
        }
        const double dlam = e[14], dgam = e[15];
        const double dg2 = tg * dgam, dtg = 2.0 * dgam;                   // d (gam^2) = 2 gam d gam, d (2 gam)
        const double dom = om1 * dchi[2];
        const double da[4] = {-dlam * chi[0] - dom * chi[1] - lam * dchi[0] - om * dchi[1],
                              dom * chi[0] - dlam * chi[1] + om * dchi[0] - lam * dchi[1],
                              dchi[3],
                              -dg2 * chi[2] - dtg * chi[3] - g2 * dchi[2] - tg * dchi[3]};
        double wda[4];
        CGP_UNROLL for (int i = 0; i < 4; i++) { wda[i] = w * da[i]; acc[i] += wda[i]; }
        CGP_UNROLL for (int i = 0; i < 4; i++)
            CGP_UNROLL for (int j = 0; j <= i; j++) {
                const int c = 4 + Sym<4>::idx(i, j);
                acc[c] = fma(dlx[i], wa[j], fma(dlx[j], wa[i], fma(lx[i], wda[j], fma(lx[j], wda[i], acc[c]))));
            }
    }
};

// What a stage needs beside its point: the trial's constants, the staged set, the LDS areas and this lane's place in the passes
struct CdSgpStageCtx {
    double lam, g2, tg, fs;              // lam, gam^2, 2 gam, fs
    Sym<4> G, dG;                        // Gamma = b b^T (replicated) and d Gamma along this lane's direction
    SigmaSet sg;
    double* red;
    double* dtab;
    int lane, s, npass, my_pass, my_slot;
    bool owner, writer, narrow;
};

// The slopes of the sigma-point moment ODE at (m, P) -- replicated -- and their tangents along this lane's direction (dm, dP): factor, the
// direction table, the fan pass by pass, as the step of sgp4_tangent_kernel.
CGP_DEV void cd_sgp4_tangent_stage(const CdSgpStageCtx& q, const double (&m)[4], const Sym<4>& P, const double (&dm)[4], const Sym<4>& dP,
                                   double (&km)[4], Sym<4>& kP, double (&dkm)[4], Sym<4>& dkP) {
    const int lane = q.lane, s = q.s;
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
    if (q.writer) {
        double* e = q.dtab + lane * kSgpDirPitch;
        CGP_UNROLL for (int i = 0; i < 4; i++) e[i] = q.owner ? dm[i] : 0.0;
        CGP_UNROLL for (int c = 0; c < Sym<4>::N; c++) e[4 + c] = q.owner ? dL.a[c] : 0.0;
    }
    wave_lds_fence();
    // ---- the fan: pass 0 = the primal sums and direction 0, pass k >= 1 = directions 2 k - 1 and 2 k; a lane takes its points two at a
    // time and, with at most 128 points, evaluates them once per stage, in pass 0
    double tp[kSgpSums], td[kSgpSums];
    CGP_UNROLL for (int c = 0; c < kSgpSums; c++) td[c] = 0.0;
    CdFanPoint pt[2];
#pragma unroll 1
    for (int pass = 0; pass < q.npass; pass++) {
        const bool first = pass == 0;
        const double* eA = q.dtab + (first ? 0 : 2 * pass - 1) * kSgpDirPitch;
        const double* eB = q.dtab + 2 * pass * kSgpDirPitch;
        double acc[2 * kSgpSums];
        CGP_UNROLL for (int c = 0; c < 2 * kSgpSums; c++) acc[c] = 0.0;
        for (int base = 0; base < s; base += 128) {
            if (first || s > 128) {
                CGP_UNROLL for (int k = 0; k < 2; k++) pt[k].eval(q.sg, base + lane + 64 * k, s, m, L, q.lam, q.g2, q.tg, q.fs);
            }
            CGP_UNROLL for (int k = 0; k < 2; k++) {
                if (first) pt[k].add_primal(acc); else pt[k].add_tangent(eA, acc, q.lam, q.g2, q.tg);
            }
            CGP_UNROLL for (int k = 0; k < 2; k++) pt[k].add_tangent(eB, acc + kSgpSums, q.lam, q.g2, q.tg);
        }
        const double* tot = coop_reduce_to_lds<2 * kSgpSums>(acc, q.red, lane, q.narrow);
        if (first) CGP_UNROLL for (int c = 0; c < kSgpSums; c++) tp[c] = tot[c];
        const bool mine = pass == q.my_pass;
        CGP_UNROLL for (int c = 0; c < kSgpSums; c++) { const double v = tot[q.my_slot + c]; td[c] = mine ? v : td[c]; }
        wave_lds_fence();
    }
    CGP_UNROLL for (int i = 0; i < 4; i++) { km[i] = tp[i]; dkm[i] = td[i]; }
    CGP_UNROLL for (int c = 0; c < Sym<4>::N; c++) { kP.a[c] = tp[4 + c] + q.G.a[c]; dkP.a[c] = td[4 + c] + q.dG.a[c]; }
}

// GAPS (CGP_SKIP_MISSING): the update gated on the step's measurement, the wavefront's one y (tangent_update<true>).  Instantiated in
// cgp_inst_gaps4_tangent_cd_sgp.hip only.
template <bool GAPS>
__global__ void __launch_bounds__(64) cd_sgp4_tangent_kernel(SgpTangentIO sio, ModelArgs ma) {
    __shared__ double red[kFanLdsDoubles];
    __shared__ __attribute__((aligned(16))) double dtab[(kSgpMaxDir + 1) * kSgpDirPitch];
    __shared__ __attribute__((aligned(16))) double park[kCdSgpParkRows * kCdSgpParkPitch];
    const TangentIO& io = sio.t;
    const int lane = threadIdx.x;
    const int64_t trial = blockIdx.x;
    if (trial >= io.B) return;

    HarmonicSDE<1> model;
    model.setup(ma.params + trial * ma.param_stride, ma.model_id);
    CdSgpStageCtx q;
    q.lam = model.lam; q.g2 = model.gam * model.gam; q.tg = 2.0 * model.gam; q.fs = model.fs;
    q.sg = ma.sg;
    q.sg.stage(dyn_lds(), lane, 64, 4);
    q.red = red; q.dtab = dtab; q.lane = lane; q.s = q.sg.s;
    q.narrow = q.s <= 32;                                                 // only lanes 0..31 hold points: half the reduction work

    // ---- this lane's direction (lanes from nd on carry a zero direction and write nothing)
    const int nd = sio.nd;
    const bool owner = lane < nd;
    q.owner = owner; q.writer = lane <= kSgpMaxDir;                       // rows nd .. kSgpMaxDir of the direction table stay zero
    q.npass = 1 + nd / 2;
    q.my_pass = (lane + 1) / 2; q.my_slot = (lane & 1) ? 0 : kSgpSums;
    double dlam = 0.0, dgam = 0.0, dXi = 0.0;
    double dm[4] = {0.0, 0.0, 0.0, 0.0};
    Sym<4> dP;
    CGP_UNROLL for (int k = 0; k < Sym<4>::N; k++) { dP.a[k] = 0.0; q.dG.a[k] = 0.0; }
    if (owner) {
        const double* __restrict__ dp = io.dirs + (trial * io.n_dir + sio.dir0 + lane) * kCdDirDoubles;
        dlam = dp[0]; dgam = dp[1];
        CGP_UNROLL for (int k = 0; k < Sym<4>::N; k++) q.dG.a[k] = dp[2 + k];
        dXi = dp[12];
        CGP_UNROLL for (int i = 0; i < 4; i++) dm[i] = dp[13 + i];
        CGP_UNROLL for (int k = 0; k < Sym<4>::N; k++) dP.a[k] = dp[17 + k];
    }
    if (q.writer) {
        double* e = dtab + lane * kSgpDirPitch;
        e[14] = dlam; e[15] = dgam;
    }
    {
        const double* __restrict__ gm = ma.gamma + trial * ma.gamma_stride;
        CGP_UNROLL for (int i = 0; i < 4; i++) CGP_UNROLL for (int j = 0; j <= i; j++) q.G(i, j) = gm[i * 4 + j];
    }
    const double dt = ma.dt, dt6 = ma.dt / 6.0;                           // h = dt / n (the host's division) and h / 6
    const int nsub = ma.substeps;

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
    const double* __restrict__ ys = io.record(trial);
    const int64_t T = io.T;
    // the parked rows: the replicated primal's (lane 0 writes it) and this owner lane's
    double* const pk = park;
    const bool parks = lane < kSgpMaxDir;                                 // (the lanes from kSgpMaxDir on read the row of zeros: their tangents stay 0)
    double* const dpk = park + (1 + (parks ? lane : kSgpMaxDir)) * kCdSgpParkPitch;
    if (lane < kCdSgpParkPitch) park[(1 + kSgpMaxDir) * kCdSgpParkPitch + lane] = 0.0;

    for (int64_t t0 = 0; t0 < T; t0 += 64) {
        const double ychunk = (t0 + lane < T) ? ys[t0 + lane] : 0.0;
        const int nsteps = (T - t0 < 64) ? (int)(T - t0) : 64;
        for (int k = 0; k < nsteps; k++) {
            const double y = readlane_f64(ychunk, k);
            // ---- nsub RK4 steps of (m, P) with its tangent (quadratures.py:49-54): x + h (k1 + 2 k2 + 2 k3 + k4) / 6
#pragma unroll 1
            for (int sub = 0; sub < nsub; sub++) {
                // park the base point and zeroed accumulators; the stage point starts as the base point and stays in registers
                if (lane == 0) {
                    CGP_UNROLL for (int i = 0; i < 4; i++) { pk[i] = m[i]; pk[14 + i] = 0.0; }
                    CGP_UNROLL for (int c = 0; c < Sym<4>::N; c++) { pk[4 + c] = P.a[c]; pk[18 + c] = 0.0; }
                }
                if (parks) {
                    CGP_UNROLL for (int i = 0; i < 4; i++) { dpk[i] = dm[i]; dpk[14 + i] = 0.0; }
                    CGP_UNROLL for (int c = 0; c < Sym<4>::N; c++) { dpk[4 + c] = dP.a[c]; dpk[18 + c] = 0.0; }
                }
                wave_lds_fence();
#pragma unroll 1
                for (int stage = 0; stage < 4; stage++) {
                    double km[4], dkm[4];
                    Sym<4> kP, dkP;
                    cd_sgp4_tangent_stage(q, m, P, dm, dP, km, kP, dkm, dkP);
                    const double wgt = (stage == 0 || stage == 3) ? 1.0 : 2.0;
                    const double hdt = (stage == 2) ? dt : 0.5 * dt;       // the next stage's point: x + h k / 2, the last one's x + h k
                    double am[4], adm[4];
                    Sym<4> aP, adP;
                    CGP_UNROLL for (int i = 0; i < 4; i++) {
                        am[i] = fma(wgt, km[i], pk[14 + i]); adm[i] = fma(wgt, dkm[i], dpk[14 + i]);
                        m[i] = fma(hdt, km[i], pk[i]); dm[i] = fma(hdt, dkm[i], dpk[i]);
                    }
                    CGP_UNROLL for (int c = 0; c < Sym<4>::N; c++) {
                        aP.a[c] = fma(wgt, kP.a[c], pk[18 + c]); adP.a[c] = fma(wgt, dkP.a[c], dpk[18 + c]);
                        P.a[c] = fma(hdt, kP.a[c], pk[4 + c]); dP.a[c] = fma(hdt, dkP.a[c], dpk[4 + c]);
                    }
                    if (stage == 3) {                                     // (uniform) the step itself: x + h / 6 (k1 + 2 k2 + 2 k3 + k4)
                        CGP_UNROLL for (int i = 0; i < 4; i++) { m[i] = fma(dt6, am[i], pk[i]); dm[i] = fma(dt6, adm[i], dpk[i]); }
                        CGP_UNROLL for (int c = 0; c < Sym<4>::N; c++) { P.a[c] = fma(dt6, aP.a[c], pk[4 + c]); dP.a[c] = fma(dt6, adP.a[c], dpk[4 + c]); }
                    } else {
                        wave_lds_fence();                                 // every lane has read the accumulators before lane 0 replaces them
                        if (lane == 0) {
                            CGP_UNROLL for (int i = 0; i < 4; i++) pk[14 + i] = am[i];
                            CGP_UNROLL for (int c = 0; c < Sym<4>::N; c++) pk[18 + c] = aP.a[c];
                        }
                        if (parks) {
                            CGP_UNROLL for (int i = 0; i < 4; i++) dpk[14 + i] = adm[i];
                            CGP_UNROLL for (int c = 0; c < Sym<4>::N; c++) dpk[18 + c] = adP.a[c];
                        }
                    }
                    wave_lds_fence();
                }
            }
            // ---- update and its tangent (the prediction is a copy: tangent_update reads it while it writes the state)
            double mp[4], dmp[4], Pp[10], dPp[10];
            CGP_UNROLL for (int i = 0; i < 4; i++) { mp[i] = m[i]; dmp[i] = dm[i]; }
            CGP_UNROLL for (int c = 0; c < Sym<4>::N; c++) { Pp[c] = P.a[c]; dPp[c] = dP.a[c]; }
            tangent_update<GAPS>(h, Xi, dXi, y, mp, dmp, Pp, dPp, m, dm, P.a, dP.a, nll, dnll);
        }
    }
    // (T == 0: nll = 0, grad = 0)
    if (nll != nll) dnll = nll;                                           // a Cholesky that broke down: NaN in value and gradient
    if (lane == 0 && sio.dir0 == 0) io.nll[trial] = nll;
    if (owner) io.grad[trial * io.n_dir + sio.dir0 + lane] = dnll;
}

template <bool GAPS>
inline hipError_t launch_cd_sgp4_tangent(const TangentIO& io, const ModelArgs& ma, hipStream_t stream) {
    return launch_tangent_slices<cd_sgp4_tangent_kernel<GAPS>>(io, ma, stream);      // (cgp_tangent4_sigma.hpp)
}

}  // namespace cgp
