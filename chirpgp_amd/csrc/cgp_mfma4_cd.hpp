// cgp_mfma4_cd.hpp -- cd_sgp_filter / cd_sgp_smoother (filters_smoothers.py:534-632) for the chirp / La Scala SDE model,
// d = 4, with the sigma-point moment ODE (filters_smoothers.py:124-137) on the float64 matrix cores (BASELINE config C4:
// Gauss-Hermite order 3, RK4, T = 50 000).
//
// Same layout and fan as cgp_mfma4_sigma.hpp: the covariance one entry per lane in the OUTPUT layout of
// v_mfma_f64_4x4x4_4b_f64 (lane (r, b, q): P[r][q]), group p = 16 s + 4 b + k evaluated by the four lanes of (k, b), the
// softplus of a group evaluated once (lane q & 1 = s) and broadcast inside the quad, nothing through LDS.  One RK4 stage:
//   * the collapsed quadrature of cgp_coop4_sigma.hpp:coop4_cd_sgp_rhs_collapsed.  The drift's last two components are
//     linear, a_2 = x_3, a_3 = -g^2 x_2 - 2 g x_3, so their expectations and the columns 2, 3 of C = E[(x - m) a^T] are
//     closed forms in (m, P): C[r][2] = P[r][3], C[r][3] = -g^2 P[r][2] - 2 g P[r][3] -- two quad broadcasts of the lane's
//     own row.  The columns 0, 1 are sums over the groups (xi_3 drops out: a_0, a_1 do not depend on it and its mean is 0),
//         C[r][q] = sum_p W_p d_r a_q,   d = L xi (xi_0..2),   a_0 = -lam c_0 - w c_1,  a_1 = w c_0 - lam c_1,  c = m + d,
//     i.e. two chained matrix instructions (A = W d_r, B = a_q) plus the sum over the four blocks, and E[a_q] two more;
//   * dP/dt = C + C^T + gamma: the transpose is one more matrix instruction (B = identity), with C + gamma riding in as its
//     accumulator;
//   * the smoother's  G^T P + P G  (filters_smoothers.py:615-621, G = Pf^{-1} gamma) is two chained matrix instructions on
//     the distributed G and P (P symmetric) instead of eight cross-lane moves and eight multiply-adds.
//   * the mean lives in COLUMN form, lane (r, b, q) holding m[q]: the RK4 bookkeeping and the mean update are one
//     instruction for all four components, E[a] comes out of the matrix instruction in that form, the fan takes m_0..3 as
//     quad broadcasts, and the smoother's G^T (m - mf) is two matrix instructions (a transpose to row form, then A = the
//     row form, B = G).
// A factorisation that fails (a pivot <= 0) poisons every output with NaN like the reference's NaN Cholesky factor does.
#pragma once
#include "cgp_mfma4_sigma.hpp"

namespace cgp {

// Per-lane constants of the moment ODE in the matrix-core layout.
struct Cd4LaneCoef {
    bool odd;                          // q & 1: the pass whose softplus this lane evaluates
    double we[2][4];                   // W_s on the component of d the lane feeds as the A operand (lane & 3), 0 elsewhere
    double k1, kn, kl0, kl1;           // a_q = (k1 w + kl0) c_0 + (kn w + kl1) c_1
    double cc2, cc3;                   // closed-form columns: C[r][q] = cc2 P[r][2] + cc3 P[r][3] for q >= 2
    double ident, gam;                 // (r == q), gamma[r][q]
    double g2, g1;                     // -g^2, -2 g
    CGP_DEV void init(int row, int q, const double (&W)[2], double lam, double g, double gamma_rq) {
        odd = (q & 1) != 0;
        CGP_UNROLL for (int s = 0; s < 2; s++) CGP_UNROLL for (int c = 0; c < 4; c++) we[s][c] = (q == c) ? W[s] : 0.0;
        k1 = (q == 1) ? 1.0 : 0.0; kn = (q == 0) ? -1.0 : 0.0;
        kl0 = (q == 0) ? -lam : 0.0; kl1 = (q == 1) ? -lam : 0.0;
        g2 = -(g * g); g1 = -2.0 * g;
        cc2 = (q == 3) ? g2 : 0.0; cc3 = (q == 2) ? 1.0 : (q == 3) ? g1 : 0.0;
        ident = (row == q) ? 1.0 : 0.0;
        gam = gamma_rq;
    }
};

// The fan of one stage: B operands a_q and A operands W d_r of both passes.
template <int MODE, bool TWO, class SM>
CGP_DEV void cd4_mfma_fan(const SM& model, const SoftplusRegs& R, const Cd4LaneCoef& K, const Fan4Groups& grp, const Sym<4>& l,
                          const double (&sd)[3], double m0, double m1, double m2, double (&a)[2], double (&wd)[2], bool& ok) {
    double c0[2], c1[2], d2[2];
    CGP_UNROLL for (int s = 0; s < (TWO ? 2 : 1); s++) {                // d = L xi, L = l diag(sd) (l unit lower), xi_3 left out
        const double xs0 = grp.xi[s][0] * sd[0], xs1 = grp.xi[s][1] * sd[1], xs2 = grp.xi[s][2] * sd[2];
        const double d1 = fma(l(1, 0), xs0, xs1);
        d2[s] = fma(l(2, 1), xs1, fma(l(2, 0), xs0, xs2));
        const double d3 = fma(l(3, 2), xs2, fma(l(3, 1), xs1, l(3, 0) * xs0));
        c0[s] = m0 + xs0; c1[s] = m1 + d1;
        wd[s] = fma(K.we[s][3], d3, fma(K.we[s][2], d2[s], fma(K.we[s][1], d1, K.we[s][0] * xs0)));   // W d_r: a select as arithmetic
    }
    typename SM::Pre pre;
    const double uv = m2 + ((TWO && K.odd) ? d2[1] : d2[0]);
    if constexpr (MODE == kFanSpec) model.precompute_spec(R, uv, pre, ok);
    else if constexpr (MODE == kFanAny) model.precompute_any(R, uv, pre, ok);
    else { model.precompute(uv, pre); ok = true; }
    const double w0 = TWO ? dpp_f64<kQuadBcast0>(pre.w) : pre.w;
    a[0] = fma(fma(K.k1, w0, K.kl0), c0[0], fma(K.kn, w0, K.kl1) * c1[0]);
    if constexpr (TWO) {
        const double w1 = dpp_f64<kQuadBcast1>(pre.w);
        a[1] = fma(fma(K.k1, w1, K.kl0), c0[1], fma(K.kn, w1, K.kl1) * c1[1]);
    }
}

// One evaluation of the sigma-point moment ODE at (m in column form, P distributed): km = E[a] in column form and the
// lane's entry of C + C^T + gamma.
// (a lane outside the lean regime [1.5, 700) sends the wavefront through the branch-free ANY fan -- round 5, cgp_models.hpp:
// precompute_any -- and only from there through the checked fan with its regime branches)
template <bool TWO, class SM>
CGP_DEV void cd4_mfma_rhs(const SM& model, const SoftplusRegs& R, const Cd4LaneCoef& K, const Fan4Groups& grp,
                          double mcol, double P, double& kmcol, double& kP) {
    // A pivot <= 0 among the first three makes its square root NaN, and through d every sum of the fan; the last pivot's
    // root is never taken (xi_3 is left out), so its sign is checked and folded into sd[2]: C, E[a] -- all entries,
    // their zero columns included (0 x NaN) -- and with them every output turn NaN, as the reference's NaN factor does
    Sym<4> l; double sd[3], dv[4];
    mfma4_factor(P, l, sd, dv);
    sd[2] += (dv[3] > 0.0) ? 0.0 : __builtin_nan("");
    const double m0 = row_bcast_f64<0>(mcol), m1 = row_bcast_f64<1>(mcol), m2 = row_bcast_f64<2>(mcol), m3 = row_bcast_f64<3>(mcol);
    double a[2], wd[2]; bool ok;
    cd4_mfma_fan<kFanSpec, TWO>(model, R, K, grp, l, sd, m0, m1, m2, a, wd, ok);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0, 0)) {
        cd4_mfma_fan<kFanAny, TWO>(model, R, K, grp, l, sd, m0, m1, m2, a, wd, ok);
        if (__builtin_amdgcn_ballot_w64(!ok) != 0) cd4_mfma_fan<kFanChecked, TWO>(model, R, K, grp, l, sd, m0, m1, m2, a, wd, ok);
    }
    double C = mfma4x4(wd[0], a[0], 0.0);
    double F = mfma4x4(grp.W[0], a[0], 0.0);
    if constexpr (TWO) {
        C = mfma4x4(wd[1], a[1], C);
        F = mfma4x4(grp.W[1], a[1], F);
    }
    C = blk_allreduce(C);                                                // sum_p W d_r a_q   (columns 0, 1; zero elsewhere)
    F = blk_allreduce(F);                                                // sum_p W a_q, in every row (zero for q >= 2)
    kmcol = fma(K.cc2, m2, fma(K.cc3, m3, F));                           // E[a_2] = m_3, E[a_3] = -g^2 m_2 - 2 g m_3: the closed-form columns' coefficients
    const double P2 = row_bcast_f64<2>(P), P3 = row_bcast_f64<3>(P);      // P[r][2], P[r][3]
    const double Cf = C + fma(K.cc2, P2, K.cc3 * P3);
    kP = mfma4x4(Cf, K.ident, Cf + K.gam);                               // C^T + (C + gamma)
}

// Scalar-measurement update (filters_smoothers.py:55-68) in the matrix-core layout: three matrix instructions (see
// cgp_mfma4_sigma.hpp); the mean in column form (Hq = H[q]: H f is a sum over the quad).
// GAPS (CGP_SKIP_MISSING): a NaN measurement zeroes the gain's reciprocal and the innovation -- Pf = Pp and mf = mp exactly, as in
// scalar_update (cgp_math.hpp); y is wave-uniform, so the gate is one condition and two selects.
template <bool GAPS = false>
CGP_DEV void mfma4_update_col(double Pp, double fcol, double Hk, double Hq, double Xi, double y,
                              double& P, double& ucol, double& S, double& innov) {
    const double PHc = mfma4x4(Hk, Pp, 0.0);                             // (Pp H^T)[q] in every row
    const double PHr = mfma4x4(Pp, Hk, 0.0);                             // (Pp H^T)[r] in every column
    S = mfma4x4(Hk, PHr, Xi);                                            // H Pp H^T + Xi
    double pred = Hq * fcol;
    pred += dpp_f64<kQuadSwap1>(pred);
    pred += dpp_f64<kQuadSwap2>(pred);
    innov = y - pred;
    double rS = rcp_nr1(S), dy = innov;
    if constexpr (GAPS) {
        const bool gap = is_missing(y);
        rS = gap ? 0.0 : rS;
        dy = gap ? 0.0 : innov;
    }
    P = fma(-(PHr * rS), PHc, Pp);                                       // Pf = Pp - K (Pp H)^T
    ucol = fma(PHc, rS * dy, fcol);                                      // mf = mp + K innov
}

// ------------------------------------------------------------------------------------------------ cd_sgp_filter, d = 4
// SUB (CGP_RK4_SUBSTEPS): n = ma.substeps RK4 steps of ma.dt = h (divided once on the host) per sample,
// a rolled loop around the same stage function; whole records only.  Instantiated in cgp_inst_substeps4.hip only.
// TIMED (include/chirpgp_hip_timed.h): the step's interval is the record's own, dts[t] -- the chunk's 64 loaded beside its measurements,
// one readlane per step, and with SUB one division by n per lane and chunk (h_t = dts[t] / n, correctly rounded); ma.dt is not read.
// Whole records only.  Instantiated in cgp_inst_timed4.hip only.
template <class SM, bool TWO, bool SPLIT, bool GAPS = false, bool SUB = false, bool TIMED = false>
// (TIMED with two passes and substeps: the allocator, left alone, takes 255 registers and 2 - 4 accumulation registers more, one wavefront per
// SIMD where the untimed sibling holds two -- 18 % at two trials per SIMD; asked for two it needs 237 - 239 and no scratch.  1: no request)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((TIMED && TWO && SUB) ? 2 : 1)))
cdsgp4_mfma_kernel(FilterIO io, ModelArgs ma) {
    static_assert(!(SPLIT && GAPS), "the time-split launches know no gaps");
    static_assert(!(SPLIT && SUB), "the time-split launches take one RK4 step per sample");
    static_assert(!(SPLIT && TIMED), "the time-split launches take one dt");
    static_assert(SM::D == 4, "d = 4 kernel");
    __shared__ double2 park[64];                                         // (S, innovation) of the chunk's steps, for the NLL
    const int lane = threadIdx.x;
    const int r = lane >> 4, b = (lane >> 2) & 3, q = lane & 3;
    const FilterSpan span = filter_span<SPLIT>(io, blockIdx.x);          // (a time-split launch: one SEGMENT of the trial's record)
    using Seg = SegRecord<4>;
    const int64_t trial = span.trial;
    if (trial >= io.B) return;

    SM model;
    model.setup(ma.params + trial * ma.param_stride, ma.model_id);
    model.wide = true;
    SigmaSet sg = ma.sg;
    sg.stage(dyn_lds(), lane, 64, 4);
    Fan4Groups grp;
    grp.template load<TWO>(sg, r, b);
    Cd4LaneCoef K;
    K.init(r, q, grp.W, model.lam, model.gam, coop4_load_sym_entry(ma.gamma + trial * ma.gamma_stride, r, q));
    SoftplusRegs R;
    R.init();
    const double* __restrict__ Hp = io.H + trial * io.H_stride;
    const double Hk = Hp[r], Hq = Hp[q];                                 // H[k] for the lane's k = lane >> 4 (A or B operand); H[q]
    const double Xi = io.Xi[trial * io.Xi_stride];
    const double dt = ma.dt;

    double u = io.m0[trial * io.m0_stride + q];                          // the mean in column form
    double P = coop4_load_sym_entry(io.P0 + trial * io.P0_stride, r, q);
    const double* __restrict__ ys = io.record(trial);
    const double* __restrict__ dtr = nullptr;
    if constexpr (TIMED) dtr = io.intervals(trial);
    Tile4FilterOut out;
    out.init(io, trial, lane);
    // (the struct's own offsets, formed before this kernel's lane range is known, cost its <false, true> form a register: 229 -> 230)
    const unsigned offP = (b == 0) ? (unsigned)(4 * r + q) * 8u : kOobOffset;
    const unsigned offm = (lane < 4) ? (unsigned)lane * 8u : kOobOffset;

    double cum = 0.0;
    for (int64_t t0 = span.t_begin; t0 < span.t_end; t0 += 64) {
        double ychunk = (t0 + lane < span.t_end) ? ys[t0 + lane] : 0.0;
        asm volatile("" : "+v"(ychunk));
        double dtchunk = 0.0;
        if constexpr (TIMED) {
            dtchunk = (t0 + lane < span.t_end) ? dtr[t0 + lane] : 0.0;
            if constexpr (SUB) dtchunk = dtchunk / (double)ma.substeps;      // h_t of the chunk's 64 steps at once: a step's own stays a readlane
            asm volatile("" : "+v"(dtchunk));
        }
        const int nsteps = (span.t_end - t0 < 64) ? (int)(span.t_end - t0) : 64;
        const bool burn = t0 < span.t_out;                               // burn-in chunks of a segment write nothing
        const OobWindow wPc = out.P_window(burn), wmc = out.m_window(burn);
        if (span.state && span.seg > 0 && t0 == span.t_out) {            // the junction: the state the burn-in arrived at
            Seg::put_mean(span.state, Seg::kJunction, lane < 4, lane, u);
            Seg::put_cov(span.state, Seg::kJunction, b == 0, r, q, P);
        }
        for (int slot = 0; slot < nsteps; slot++) {
            const unsigned t = (unsigned)(t0 + slot);
            const double y = readlane_f64(ychunk, slot);
            double f = u, Pp = P;
            auto rhs = [&](double tm, double tP, double& km, double& kP) { cd4_mfma_rhs<TWO>(model, R, K, grp, tm, tP, km, kP); };
            if constexpr (TIMED) {
                const double h = readlane_f64(dtchunk, slot);
                if constexpr (SUB) {
#pragma unroll 1
                    for (int j = 0; j < ma.substeps; j++) rk4_lane(h, f, Pp, rhs);
                } else rk4_lane(h, f, Pp, rhs);
            } else if constexpr (SUB) {
#pragma unroll 1
                for (int j = 0; j < ma.substeps; j++) rk4_lane(dt, f, Pp, rhs);
            } else rk4_lane(dt, f, Pp, rhs);
            // ---- update
            double S, innov;
            mfma4_update_col<GAPS>(Pp, f, Hk, Hq, Xi, y, P, u, S, innov);
            park[slot] = make_double2(S, innov);                        // every lane holds them: same address, same value
            wPc.store(P, t * 128u + offP);
            wmc.store(u, t * 32u + offm);
        }
        if (out.want_nll && !burn) {
            cum = out.template flush_nll<GAPS>(park, lane, nsteps, cum, t0, ychunk);
            wave_lds_fence();
        }
    }
    if (span.state) {                                                    // the segment's last state and its NLL total, for the fix-up pass
        Seg::put_mean(span.state, Seg::kEnd, lane < 4, lane, u);
        Seg::put_cov(span.state, Seg::kEnd, b == 0, r, q, P);
        Seg::put_nll(span.state, lane, cum);
    } else out.store_nll_total(io, trial, lane, cum);
}

// THE backward loop of the continuous-discrete smoothers in this layout, for the (trial, segment) that `sio` decoded: per chunk of 64 steps
// the gains G = Pf^{-1} gamma, lane-parallel (cgp_coop4_sigma.hpp:coop4_chunk_gains), read back from LDS one entry per lane (Gd = G[r][q], and
// mf in column form); per step RK4 from t + 1 to t (dt < 0) on rhs(m, P, Gd, mf, km, kP) -- a kernel's own -- and the stores.
// SPLIT (round 6; cgp_smoother_time_split): one wavefront per (trial, segment) -- see SmootherIO::bsegs.  Chunk j covers the rows
// T - 2 - 64 j - 63 .. T - 2 - 64 j; segment s owns the chunks [s cps, (s + 1) cps) and starts burn_chunks chunks earlier in its walk
// (later in time) from the FILTERING row there; the burn-in chunks store through a zero-byte window.
// TIMED (include/chirpgp_hip_timed.h): the step from row t + 1 to row t runs over the trial's dts[t + 1] -- lane l of a chunk loads the
// interval of the chunk's slot l, dts[t_hi - l + 1], and each step takes its own by readlane and negates it; `dt` is not read.
template <bool SPLIT, bool TIMED = false, class Rhs>
CGP_DEV void cd4_mfma_smoother_walk(const SmootherIO& io, Tile4SmootherIO& sio, int lane, const Sym<4>& gamma, double dt, double* gbuf, Rhs rhs) {
    const int r = lane >> 4, q = lane & 3;
    if (!sio.template init<SPLIT>(io, lane)) return;
    const int64_t T = io.T;
    const double* __restrict__ mfs = sio.mfs;
    const double* __restrict__ Pfs = sio.Pfs;
    const SmootherSpan sp = sio.sp;
    static_assert(!(SPLIT && TIMED), "the time-split launches take one dt");
    const double* __restrict__ dtr = nullptr;
    if constexpr (TIMED) dtr = io.intervals(sio.trial);
    double ms = mfs[sp.t_start * 4 + q];                                 // the mean in column form
    double Ps = coop4_load_sym_entry(Pfs + sp.t_start * 16, r, q);

    for (int64_t j = sp.j_first; j <= sp.j_last; j++) {
        const int64_t t_hi = T - 2 - 64 * j;
        const bool own = j >= sp.j_own;
        if constexpr (SPLIT) { if (j == sp.j_own) sio.junction_store(io, lane, ms, Ps); }
        const OobWindow& oP = sio.P_window(own);
        const OobWindow& om = sio.m_window(own);
        const int nsteps = t_hi + 1 < 64 ? (int)(t_hi + 1) : 64;
        coop4_chunk_gains(gbuf, lane, nsteps, t_hi, mfs, Pfs, gamma);
        double dtchunk = 0.0;
        if constexpr (TIMED) {
            dtchunk = (lane < nsteps) ? dtr[t_hi - lane + 1] : 0.0;       // (t_hi + 1 <= T - 1: inside the grid)
            asm volatile("" : "+v"(dtchunk));
        }
        for (int slot = 0; slot < nsteps; slot++) {
            const unsigned t = (unsigned)(t_hi - slot);
            const double* gl = gbuf + slot * kGainPitch;
            const double Gd = gl[r * 4 + q];
            const double mf = gl[16 + q];
            double h = dt;
            if constexpr (TIMED) h = -readlane_f64(dtchunk, slot);
            rk4_lane(h, ms, Ps, [&](double tm, double tP, double& km, double& kP) { rhs(tm, tP, Gd, mf, km, kP); });
            oP.store(Ps, t * 128u + sio.offP);
            om.store(ms, t * 32u + sio.offm);
        }
        wave_lds_fence();
    }
}

// ------------------------------------------------------------------------------------------------ cd_sgp_smoother, d = 4
// Backward RK4 with  dm = _m + G^T (m - mf),  dP = _P + G^T P + P G - 2 gamma,  G = Pf^{-1} gamma  (filters_smoothers.py:615-621).
// G is constant over the four stages and computed a chunk of 64 steps at a time, lane-parallel (cgp_coop4_sigma.hpp:
// coop4_chunk_gains); the walk reads it back from LDS one entry per lane, and mf in column form.
// SPLIT: cd4_mfma_smoother_walk.
template <class SM, bool TWO, bool SPLIT = false, bool TIMED = false>
__global__ void __launch_bounds__(64) cdsgps4_mfma_kernel(SmootherIO io, ModelArgs ma) {
    static_assert(SM::D == 4, "d = 4 kernel");
    __shared__ __attribute__((aligned(16))) double gbuf[64 * kGainPitch];
    const int lane = threadIdx.x;
    const int r = lane >> 4, b = (lane >> 2) & 3, q = lane & 3;
    Tile4SmootherIO sio;
    sio.template decode<SPLIT>(io);
    const int64_t trial = sio.trial;
    if (trial >= io.B) return;

    SM model;
    model.setup(ma.params + trial * ma.param_stride, ma.model_id);
    model.wide = true;
    SigmaSet sg = ma.sg;
    sg.stage(dyn_lds(), lane, 64, 4);
    Fan4Groups grp;
    grp.template load<TWO>(sg, r, b);
    Sym<4> gamma;
    load_sym<4>(ma.gamma + trial * ma.gamma_stride, gamma);
    Cd4LaneCoef K;
    K.init(r, q, grp.W, model.lam, model.gam, coop4_load_sym_entry(ma.gamma + trial * ma.gamma_stride, r, q));
    SoftplusRegs R;
    R.init();
    cd4_mfma_smoother_walk<SPLIT, TIMED>(io, sio, lane, gamma, -ma.dt, gbuf, [&](double tm, double tP, double Gd, double mf, double& km, double& kP) {
        cd4_mfma_rhs<TWO>(model, R, K, grp, tm, tP, km, kP);            // (_m, _P), _P includes + gamma
        const double drow = mfma4x4(tm - mf, K.ident, 0.0);             // m - mf from column to row form: [r][q] <- [q][r]
        km = mfma4x4(drow, Gd, km);                                     // _m + G^T (m - mf): sum_k (m - mf)[k] G[k][q]   (A operand G[k][r'], B operand G[k][q'])
        const double sym = mfma4x4(Gd, tP, mfma4x4(tP, Gd, 0.0));       // G^T P + P G (P symmetric)
        kP = (kP + sym) - 2.0 * K.gam;
    });
}

// ------------------------------------------------------------------------------------------------ cd_ekf / cd_eks, d = 4
// dm = a(m), dP = J P + P J^T + gamma (filters_smoothers.py:384-394) and the smoother's dm = a(m) + G^T (m - mf),
// dP = A P + P A^T - gamma, A = J + G^T (filters_smoothers.py:427-438) in the same layout: the drift Jacobian
//     J_a = [[-lam, -w, -dw u1, 0], [w, -lam, dw u0, 0], [0, 0, 0, 1], [0, 0, -g^2, -2 g]]    
// is held TRANSPOSED, one entry per lane (lane (r, b, q): J[q][r], i.e. the A operand "J[r'][k]"), assembled from the
// wave-uniform (w, dw) with per-lane 0 / +-1 / constant coefficients; then J P is ONE matrix instruction and
// (J P)^T + J P + gamma another (B = identity, the accumulator carries J P + gamma).  G enters A^T as the lane's own G[r][q].
struct Cd4JacCoef {
    double cb, cg0, cg1, ck;           // J[q][r] = cb w + cg0 jv0 + cg1 jv1 + ck
    CGP_DEV void init(int r, int q, double lam, double g) {
        cb = (q == 0 && r == 1) ? -1.0 : (q == 1 && r == 0) ? 1.0 : 0.0;
        cg0 = (q == 0 && r == 2) ? 1.0 : 0.0; cg1 = (q == 1 && r == 2) ? 1.0 : 0.0;
        ck = ((q == 0 && r == 0) || (q == 1 && r == 1)) ? -lam : (q == 2 && r == 3) ? 1.0 : (q == 3 && r == 2) ? -(g * g) : (q == 3 && r == 3) ? -2.0 * g : 0.0;
    }
};
// a(m) in column form and the lane's entry of J^T at the mean (column form in, quad broadcasts).
CGP_DEV void cd4_ekf_eval(const SoftplusRegs& R, const Cd4LaneCoef& K, const Cd4JacCoef& Jc, double fs, double mcol, double& acol, double& JT) {
    const double m0 = row_bcast_f64<0>(mcol), m1 = row_bcast_f64<1>(mcol), m2 = row_bcast_f64<2>(mcol), m3 = row_bcast_f64<3>(mcol);
    double sp, dsp;
    softplus_pair_uniform(R, m2, sp, dsp);
    const double w = (kTwoPi * sp) * fs, dw = (kTwoPi * dsp) * fs;
    acol = fma(fma(K.k1, w, K.kl0), m0, fma(K.kn, w, K.kl1) * m1) + fma(K.cc2, m2, K.cc3 * m3);
    const double jv0 = -dw * m1, jv1 = dw * m0;
    JT = fma(Jc.cb, w, fma(Jc.cg0, jv0, fma(Jc.cg1, jv1, Jc.ck)));
}

#ifndef CGP_NO_CD_EKF_KERNELS       // the kernels below are instantiated in cgp_inst_mfma4.hip (GAPS: cgp_inst_gaps4_sigma.hip)
// SUB (CGP_RK4_SUBSTEPS): n = ma.substeps RK4 steps of ma.dt = h (divided once on the host) per sample, a rolled loop
// around the same stage function; the NLL flush and the stores go by samples as before.  Instantiated in cgp_inst_substeps4.hip only.
// TIMED: as in cdsgp4_mfma_kernel.  Instantiated in cgp_inst_timed4.hip only.
template <bool GAPS = false, bool SUB = false, bool TIMED = false>
__global__ void __launch_bounds__(64) cdekf4_mfma_kernel(FilterIO io, ModelArgs ma) {
    __shared__ double2 park[64];                                         // (S, innovation) of the chunk's steps, for the NLL
    const int lane = threadIdx.x;
    const int r = lane >> 4, q = lane & 3;
    const int64_t trial = blockIdx.x;
    if (trial >= io.B) return;

    HarmonicSDE<1> model;
    model.setup(ma.params + trial * ma.param_stride, ma.model_id);
    const double W0[2] = {0.0, 0.0};
    Cd4LaneCoef K;
    K.init(r, q, W0, model.lam, model.gam, coop4_load_sym_entry(ma.gamma + trial * ma.gamma_stride, r, q));
    Cd4JacCoef Jc;
    Jc.init(r, q, model.lam, model.gam);
    SoftplusRegs R;
    R.init();
    const double* __restrict__ Hp = io.H + trial * io.H_stride;
    const double Hk = Hp[r], Hq = Hp[q];
    const double Xi = io.Xi[trial * io.Xi_stride];
    const double dt = ma.dt, fs = model.fs;

    double u = io.m0[trial * io.m0_stride + q];                          // the mean in column form
    double P = coop4_load_sym_entry(io.P0 + trial * io.P0_stride, r, q);
    const int64_t T = io.T;
    const double* __restrict__ ys = io.record(trial);
    const double* __restrict__ dtr = nullptr;
    if constexpr (TIMED) dtr = io.intervals(trial);
    Tile4FilterOut out;
    out.init(io, trial, lane);

    double cum = 0.0;
    for (int64_t t0 = 0; t0 < T; t0 += 64) {
        double ychunk = (t0 + lane < T) ? ys[t0 + lane] : 0.0;
        asm volatile("" : "+v"(ychunk));
        double dtchunk = 0.0;
        if constexpr (TIMED) {
            dtchunk = (t0 + lane < T) ? dtr[t0 + lane] : 0.0;
            if constexpr (SUB) dtchunk = dtchunk / (double)ma.substeps;      // h_t of the chunk's 64 steps at once: a step's own stays a readlane
            asm volatile("" : "+v"(dtchunk));
        }
        const int nsteps = (T - t0 < 64) ? (int)(T - t0) : 64;
        for (int slot = 0; slot < nsteps; slot++) {
            const unsigned t = (unsigned)(t0 + slot);
            const double y = readlane_f64(ychunk, slot);
            double f = u, Pp = P;
            auto rhs = [&](double tm, double tP, double& km, double& kP) {
                double JT;
                cd4_ekf_eval(R, K, Jc, fs, tm, km, JT);
                const double JP = mfma4x4(JT, tP, 0.0);                  // sum_k J[r][k] P[k][q]
                kP = mfma4x4(JP, K.ident, JP + K.gam);                   // (J P)^T + J P + gamma
            };
            if constexpr (TIMED) {
                const double h = readlane_f64(dtchunk, slot);
                if constexpr (SUB) {
#pragma unroll 1
                    for (int j = 0; j < ma.substeps; j++) rk4_lane(h, f, Pp, rhs);
                } else rk4_lane(h, f, Pp, rhs);
            } else if constexpr (SUB) {
#pragma unroll 1
                for (int j = 0; j < ma.substeps; j++) rk4_lane(dt, f, Pp, rhs);
            } else rk4_lane(dt, f, Pp, rhs);
            double S, innov;
            mfma4_update_col<GAPS>(Pp, f, Hk, Hq, Xi, y, P, u, S, innov);
            park[slot] = make_double2(S, innov);
            out.wP.store(P, t * 128u + out.offP);
            out.wm.store(u, t * 32u + out.offm);
        }
        if (out.want_nll) {
            cum = out.template flush_nll<GAPS>(park, lane, nsteps, cum, t0, ychunk);
            wave_lds_fence();
        }
    }
    out.store_nll_total(io, trial, lane, cum);
}

template <bool SPLIT = false, bool TIMED = false>      // SPLIT: cgp_smoother_time_split, as cdsgps4_mfma_kernel; TIMED: cd4_mfma_smoother_walk
__global__ void __launch_bounds__(64) cdeks4_mfma_kernel(SmootherIO io, ModelArgs ma) {
    __shared__ __attribute__((aligned(16))) double gbuf[64 * kGainPitch];
    const int lane = threadIdx.x;
    const int r = lane >> 4, q = lane & 3;
    Tile4SmootherIO sio;
    sio.template decode<SPLIT>(io);
    const int64_t trial = sio.trial;
    if (trial >= io.B) return;

    HarmonicSDE<1> model;
    model.setup(ma.params + trial * ma.param_stride, ma.model_id);
    const double W0[2] = {0.0, 0.0};
    Cd4LaneCoef K;
    K.init(r, q, W0, model.lam, model.gam, coop4_load_sym_entry(ma.gamma + trial * ma.gamma_stride, r, q));
    Cd4JacCoef Jc;
    Jc.init(r, q, model.lam, model.gam);
    SoftplusRegs R;
    R.init();
    Sym<4> gamma;
    load_sym<4>(ma.gamma + trial * ma.gamma_stride, gamma);
    const double fs = model.fs;
    cd4_mfma_smoother_walk<SPLIT, TIMED>(io, sio, lane, gamma, -ma.dt, gbuf, [&](double tm, double tP, double Gd, double mf, double& km, double& kP) {
        double JT;
        cd4_ekf_eval(R, K, Jc, fs, tm, km, JT);
        const double drow = mfma4x4(tm - mf, K.ident, 0.0);             // m - mf from column to row form
        km = mfma4x4(drow, Gd, km);                                     // a(m) + G^T (m - mf)
        const double AP = mfma4x4(JT + Gd, tP, 0.0);                    // sum_k A[r][k] P[k][q], A = J + G^T: G[r][q] = (G^T)[q][r] is the lane's entry of A^T - J^T
        kP = mfma4x4(AP, K.ident, AP - K.gam);                          // (A P)^T + A P - gamma
    });
}

template <bool GAPS = false>
inline int launch_cdekf4_mfma(const FilterIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return CGP_OK;
    if (!mfma4_rows_fit(io.T)) return CGP_E_UNSUPPORTED;
    hipLaunchKernelGGL(cdekf4_mfma_kernel<GAPS>, dim3((unsigned)io.B), dim3(64), 0, stream, io, ma);
    return hip_rc(hipGetLastError());
}
template <bool GAPS>
inline int launch_cdekf4_mfma_substeps(const FilterIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return CGP_OK;
    if (!mfma4_rows_fit(io.T)) return CGP_E_UNSUPPORTED;
    hipLaunchKernelGGL((cdekf4_mfma_kernel<GAPS, true>), dim3((unsigned)io.B), dim3(64), 0, stream, io, ma);
    return hip_rc(hipGetLastError());
}
// timed calls (cgp_inst_timed4.hip, cgp_inst_timed4_smoothers.hip): whole records, one wavefront per trial
template <bool GAPS, bool SUB>
inline int launch_cdekf4_mfma_timed(const FilterIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return CGP_OK;
    if (!mfma4_rows_fit(io.T) || !io.dts) return CGP_E_UNSUPPORTED;
    hipLaunchKernelGGL((cdekf4_mfma_kernel<GAPS, SUB, true>), dim3((unsigned)io.B), dim3(64), 0, stream, io, ma);
    return hip_rc(hipGetLastError());
}
template <bool TIMED = true>         // (a template, so that only the unit that calls it holds the kernel)
inline int launch_cdeks4_mfma_timed(const SmootherIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return CGP_OK;
    if (!mfma4_rows_fit(io.T) || io.bsegs > 1 || !io.dts) return CGP_E_UNSUPPORTED;
    hipLaunchKernelGGL((cdeks4_mfma_kernel<false, TIMED>), dim3((unsigned)io.B), dim3(64), 0, stream, io, ma);
    return hip_rc(hipGetLastError());
}
#ifndef CGP_NO_UNTIMED_CD_EKS      // (not a template: every unit that sees it holds its two kernels; the units of the timed kernels leave it out)
inline int launch_cdeks4_mfma(const SmootherIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return CGP_OK;
    if (!mfma4_rows_fit(io.T)) return CGP_E_UNSUPPORTED;
    if (io.bsegs > 1) {
        if (io.B * io.bsegs > 0x7fffffffLL) return CGP_E_UNSUPPORTED;
        hipLaunchKernelGGL(cdeks4_mfma_kernel<true>, dim3((unsigned)(io.B * io.bsegs)), dim3(64), 0, stream, io, ma);
    } else {
        hipLaunchKernelGGL(cdeks4_mfma_kernel<false>, dim3((unsigned)io.B), dim3(64), 0, stream, io, ma);
    }
    return hip_rc(hipGetLastError());
}
#endif  // CGP_NO_UNTIMED_CD_EKS
#endif  // CGP_NO_CD_EKF_KERNELS

template <class SM, bool GAPS = false>
inline int launch_cdsgp4_mfma(const FilterIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return CGP_OK;
    if (!sgp4_mfma_fits(io.T, ma)) return CGP_E_UNSUPPORTED;
    const bool two = ma.sg.n_groups > 16;
    if constexpr (GAPS) {                                                           // (CGP_SKIP_MISSING: whole records only, route_filter)
        if (io.segs > 1) return CGP_E_UNSUPPORTED;
        if (two) hipLaunchKernelGGL((cdsgp4_mfma_kernel<SM, true, false, true>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
        else hipLaunchKernelGGL((cdsgp4_mfma_kernel<SM, false, false, true>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
        return hip_rc(hipGetLastError());
    }
    if (io.segs > 1) {                                                              // time-split: one wavefront per (trial, segment)
        const unsigned grid = (unsigned)(io.B * io.segs);
        if (two) hipLaunchKernelGGL((cdsgp4_mfma_kernel<SM, true, true>), dim3(grid), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
        else hipLaunchKernelGGL((cdsgp4_mfma_kernel<SM, false, true>), dim3(grid), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    } else if (two) hipLaunchKernelGGL((cdsgp4_mfma_kernel<SM, true, false>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    else hipLaunchKernelGGL((cdsgp4_mfma_kernel<SM, false, false>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    return hip_rc(hipGetLastError());
}
template <class SM, bool GAPS>
inline int launch_cdsgp4_mfma_substeps(const FilterIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return CGP_OK;
    if (!sgp4_mfma_fits(io.T, ma) || io.segs > 1) return CGP_E_UNSUPPORTED;          // (whole records only, route_filter)
    if (ma.sg.n_groups > 16) hipLaunchKernelGGL((cdsgp4_mfma_kernel<SM, true, false, GAPS, true>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    else hipLaunchKernelGGL((cdsgp4_mfma_kernel<SM, false, false, GAPS, true>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    return hip_rc(hipGetLastError());
}
template <class SM, bool GAPS, bool SUB>
inline int launch_cdsgp4_mfma_timed(const FilterIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return CGP_OK;
    if (!sgp4_mfma_fits(io.T, ma) || io.segs > 1 || !io.dts) return CGP_E_UNSUPPORTED;
    if (ma.sg.n_groups > 16) hipLaunchKernelGGL((cdsgp4_mfma_kernel<SM, true, false, GAPS, SUB, true>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    else hipLaunchKernelGGL((cdsgp4_mfma_kernel<SM, false, false, GAPS, SUB, true>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    return hip_rc(hipGetLastError());
}
template <class SM>
inline int launch_cdsgps4_mfma_timed(const SmootherIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return CGP_OK;
    if (!sgp4_mfma_fits(io.T, ma) || io.bsegs > 1 || !io.dts) return CGP_E_UNSUPPORTED;
    if (ma.sg.n_groups > 16) hipLaunchKernelGGL((cdsgps4_mfma_kernel<SM, true, false, true>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    else hipLaunchKernelGGL((cdsgps4_mfma_kernel<SM, false, false, true>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    return hip_rc(hipGetLastError());
}
template <class SM>
inline int launch_cdsgps4_mfma(const SmootherIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return CGP_OK;
    if (!sgp4_mfma_fits(io.T, ma)) return CGP_E_UNSUPPORTED;
    if (io.bsegs > 1) {                                                             // time-split with burn-in: one wavefront per (trial, segment)
        const unsigned grid = (unsigned)(io.B * io.bsegs);
        if (ma.sg.n_groups > 16) hipLaunchKernelGGL((cdsgps4_mfma_kernel<SM, true, true>), dim3(grid), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
        else hipLaunchKernelGGL((cdsgps4_mfma_kernel<SM, false, true>), dim3(grid), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
        return hip_rc(hipGetLastError());
    }
    if (ma.sg.n_groups > 16) hipLaunchKernelGGL((cdsgps4_mfma_kernel<SM, true>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    else hipLaunchKernelGGL((cdsgps4_mfma_kernel<SM, false>), dim3((unsigned)io.B), dim3(64), sigma_lds_bytes(ma, 4), stream, io, ma);
    return hip_rc(hipGetLastError());
}

}  // namespace cgp
