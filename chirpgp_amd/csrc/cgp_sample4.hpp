// cgp_sample4.hpp -- posterior sample paths of the discrete smoothers (rts / eks / sgp_smoother) for d = 4 by backward simulation
// (forward filtering, backward sampling): cgp_smoother_sample of include/chirpgp_hip.h.
//
// The law.  The smoothers' backward recursion is an affine map per step whose coefficients depend on the filtering rows only
// (cgp_walk4.hpp):   ms_t = G_t ms_{t+1} + c_t,   Ps_t = G_t Ps_{t+1} G_t^T + C_t,   c_t = mf_t - G_t mp_t,   C_t = Pf_t - G_t Pp_t G_t^T.
// The same (G_t, c_t, C_t) are the backward kernel of the Gauss-Markov posterior those moments belong to,
//     x_t | x_{t+1} ~ N(c_t + G_t x_{t+1}, C_t),
// so a path is ONE backward walk of the smoother's map with noise added at every step:
//     x_{T-1} = mf_{T-1} + L(Pf_{T-1}) z_{T-1},        x_t = c_t + G_t x_{t+1} + L(C_t) z_t,   t = T - 2 .. 0,        z_t ~ N(0, I).
// Sample mean, covariance and lag-one cross-covariance of the paths converge to mss, Pss and G_t Pss_{t+1}: the joint law, which
// independent draws from the marginals do not have.
//
// The pivot rule (a definition, not a tolerance).  L(A) is the lower-triangular Cholesky factor of A, column by column; in the
// factorisation of C_t a pivot   p_j = C_t[j][j] - sum_{k<j} L[j][k]^2   with   p_j <= 2^-40 Pf_t[j][j]   makes COLUMN j of L zero, and the
// same holds for Pf_{T-1} against its own diagonal.  The chirp block of the La Scala model has no process noise: the EKS's C_t has rank 2
// in exact arithmetic and a plain factorisation returns NaN or rounding noise; with the rule those components are deterministic given
// x_{t+1}, and the variance dropped is at most 2^-40 of the filtering variance.  A NaN pivot compares false and stays NaN: a broken
// filtering row gives NaN paths from there back, as the smoothers do.  The tests restate the rule operation by operation.
//
// The kernel.  One wavefront per (trial, group of 64 samples) walks tiles of 64 steps backwards:
//   phase G  (lane = time step)  phase G of walk4_smoother_kernel: every lane builds the map of ITS step -- Elem's prediction at (mf_t, Pf_t), the gain in full float64, for a linear model C_t in the Joseph form (sample_map) -- factors
//            C_t and parks (G_t, c_t, L_t) in LDS: 16 + 4 + 10 doubles, record stride 31 (odd: conflict-free lane stride), 15.9 KB a tile;
//   phase W  (lane = sample)  the 64 lanes carry 64 samples of the trial through the tile's steps in order; every lane reads the SAME record
//            at a step (a broadcast read), draws its own z_t and applies the map: 26 multiply-adds a step, then stores its row
//            paths[b][s][t][0 .. 3] (32 bytes) and / or comp_paths[b][s][t].  The step loop is kept rolled: one copy of the generator.
// Sample groups beyond the first take the second grid dimension and rebuild the records (phase G is one map per lane and tile, phase W
// 64 steps of two Philox blocks and two Box-Muller pairs per lane: a few per cent), which also spreads ONE record's samples over the
// machine; a wavefront that walked several groups over the same records would keep one carry per group and is not built.
//
// The random stream (cgp_rng.hpp, kStreamPosterior): component j of z_t of sample s of trial b is member j & 1 of
//     normal_pair(seed, (trial0 + b) | (uint64_t)(sample0 + s) << 32, index = 2 t + (j >> 1), kStreamPosterior)
// -- a path depends on (seed, global trial, global sample) only, never on B, S or the launch shape.  With `normals` the caller's z is
// read instead ([B][S][T][4]).
#pragma once
#include "cgp_kernels.hpp"
#include <type_traits>
#include "cgp_rng.hpp"

namespace cgp {

constexpr int kSampRec = 31;                      // G 16 (row-major) | c 4 | L 10 (packed lower triangle, Sym<4>::idx) | pad: odd
constexpr int kSampG = 0, kSampc = 16, kSampL = 20;
constexpr double kSamplePivotFloor = 0x1p-40;     // a pivot <= this x the filtering variance of its component: the column is zero


// L L^T = A under the pivot rule, `ref` the matrix whose diagonal the pivots are held against
template <int D>
CGP_DEV void cholesky_pivot_rule(const Sym<D>& A, const Sym<D>& ref, Sym<D>& L) {
    CGP_UNROLL for (int j = 0; j < D; j++) {
        double p = A(j, j);
        CGP_UNROLL for (int k = 0; k < j; k++) p = fma(-L(j, k), L(j, k), p);
        const bool drop = p <= kSamplePivotFloor * ref(j, j);             // (NaN: false)
        const double ljj = drop ? 0.0 : sqrt(p);
        L(j, j) = ljj;
        CGP_UNROLL for (int i = j + 1; i < D; i++) {
            double t = A(i, j);
            CGP_UNROLL for (int k = 0; k < j; k++) t = fma(-L(i, k), L(j, k), t);
            L(i, j) = drop ? 0.0 : t / ljj;
        }
    }
}

// The step's affine map (G, c, C) from Elem's own prediction -- what Elem::map builds, with the gain solved in full float64: IEEE square
// roots and divisions instead of sqrt_rsqrt's 5e-15 (cgp_math.hpp), which the smoothers can afford and this walk cannot.  C = Pf - G D^T
// is a difference of nearly equal numbers wherever the process noise is small (a pivot of 7e-9 beside Pf = 0.3 in the chirp models'
// frequency state), and L(C) carries the pivot's RELATIVE error: an absolute 1e-14 in G D^T is 1e-6 of that pivot, 3e-10 of a path.
template <int D>
CGP_DEV void gain_full_precision(const Sym<D>& Pp, const Mat<D>& DT, Mat<D>& G) {
    Sym<D> L;
    bool bad = false;
    CGP_UNROLL for (int j = 0; j < D; j++) {
        double s = Pp(j, j);
        CGP_UNROLL for (int k = 0; k < j; k++) s = fma(-L(j, k), L(j, k), s);
        bad = bad || !(s > 0.0);
        L(j, j) = sqrt(s);
        CGP_UNROLL for (int i = j + 1; i < D; i++) {
            double t = Pp(i, j);
            CGP_UNROLL for (int k = 0; k < j; k++) t = fma(-L(i, k), L(j, k), t);
            L(i, j) = t / L(j, j);
        }
    }
    const double poison = bad ? __builtin_nan("") : 0.0;                  // a prediction that is not positive definite: NaN, as cholesky()
    CGP_UNROLL for (int c = 0; c < D; c++) {                              // row c of G solves (L L^T) x = DT[:, c]: one rounding per division
        double x[D];
        CGP_UNROLL for (int i = 0; i < D; i++) {
            double s = DT.a[i][c];
            CGP_UNROLL for (int k = 0; k < i; k++) s = fma(-L(i, k), x[k], s);
            x[i] = s / L(i, i);
        }
        CGP_UNROLL for (int i = D - 1; i >= 0; i--) {
            double s = x[i];
            CGP_UNROLL for (int k = i + 1; k < D; k++) s = fma(-L(k, i), x[k], s);
            x[i] = s / L(i, i);
        }
        CGP_UNROLL for (int i = 0; i < D; i++) G.a[c][i] = x[i] + poison;
    }
}
template <class Elem>
CGP_DEV void sample_map(const Elem& e, const Vec<Elem::D>& mf, const Sym<Elem::D>& Pf, Mat<Elem::D>& G, Vec<Elem::D>& c, Sym<Elem::D>& C) {
    constexpr int D = Elem::D;
    Mat<D> DT; Vec<D> mp; Sym<D> Pp;
    if constexpr (Elem::USES_SIGMA) sgp_prediction<decltype(e.model), false, true, true, false>(e.model, e.sg, 0, nullptr, mf, Pf, mp, Pp, DT);
    else e.model.propagate(mf, Pf, mp, DT, Pp);
    gain_full_precision<D>(Pp, DT, G);
    if constexpr (std::is_same<typename std::decay<decltype(e.model)>::type, LinearDisc<D>>::value && !Elem::USES_SIGMA) {
        // a linear model hands over F and Sigma themselves: the Joseph form  C = A Pf A^T + G Sigma G^T,  c = A mf,  A = I - G F  -- sums of
        // positive terms where Pf - G D^T cancels (the small pivots then come from G Sigma G^T at Sigma's own relative accuracy)
        Mat<D> A, W, GS;
        CGP_UNROLL for (int i = 0; i < D; i++)
            CGP_UNROLL for (int j = 0; j < D; j++) {
                double a = (i == j) ? 1.0 : 0.0;
                CGP_UNROLL for (int k = 0; k < D; k++) a = fma(-G.a[i][k], e.model.F.a[k][j], a);
                A.a[i][j] = a;
            }
        CGP_UNROLL for (int i = 0; i < D; i++) {
            double a = 0.0;
            CGP_UNROLL for (int k = 0; k < D; k++) a = fma(A.a[i][k], mf.v[k], a);
            c.v[i] = a;
            CGP_UNROLL for (int j = 0; j < D; j++) {
                double w = 0.0, g = 0.0;
                CGP_UNROLL for (int k = 0; k < D; k++) { w = fma(A.a[i][k], Pf(k, j), w); g = fma(G.a[i][k], e.model.Sigma(k, j), g); }
                W.a[i][j] = w; GS.a[i][j] = g;
            }
        }
        CGP_UNROLL for (int i = 0; i < D; i++)
            CGP_UNROLL for (int j = 0; j <= i; j++) {
                double a = 0.0;
                CGP_UNROLL for (int k = 0; k < D; k++) a = fma(GS.a[i][k], G.a[j][k], a);
                CGP_UNROLL for (int k = 0; k < D; k++) a = fma(W.a[i][k], A.a[j][k], a);
                C(i, j) = a;
            }
    } else {
        map_from_gain<D>(mf, Pf, mp, Pp, DT, G, c, C);
    }
}

// func(x) of cgp_sample_out: the integrands of cgp_gaussian_expectation_fn, pointwise
CGP_DEV double sample_fn(int func, double x) {
    if (func == CGP_FN_SOFTPLUS) { const double e = exp(x); return x < 0.0 ? log1p(e) : log(e + 1.0); }      // as gh_expectation (cgp_kernels.hpp) evaluates it
    if (func == CGP_FN_EXP) return exp(x);
    if (func == CGP_FN_SQUARE) return x * x;
    return x;
}

template <class Elem>
__global__ void __launch_bounds__(64) sample4_kernel(SampleIO io, ModelArgs ma) {
    static_assert(Elem::D == 4, "d = 4 kernel");
    __shared__ double recs[64 * kSampRec];
    const int lane = threadIdx.x;
    const int64_t trial = blockIdx.x;
    if (trial >= io.B) return;
    const int64_t T = io.T;

    Elem elem;
    elem.setup(ma, trial);
    if constexpr (Elem::USES_SIGMA) { elem.sg.stage(dyn_lds(), lane, 64, 4); wave_lds_fence(); }
    const double* __restrict__ mfs = io.mfs + trial * T * 4;
    const double* __restrict__ Pfs = io.Pfs + trial * T * 16;
    const int64_t groups = (io.S + 63) / 64;

    for (int64_t group = blockIdx.y; group < groups; group += gridDim.y) {
        const int64_t s = group * 64 + lane;
        const bool live = s < io.S;                                       // (a lane without a sample still builds its step's record)
        const int64_t row = (trial * io.S + (live ? s : 0)) * T;          // first step of the lane's path, in steps
        const double* __restrict__ zs = io.normals ? io.normals + row * 4 : nullptr;
        double* __restrict__ px = (io.paths && live) ? io.paths + row * 4 : nullptr;
        double* __restrict__ pc = (io.comp_paths && live) ? io.comp_paths + row : nullptr;
        const uint64_t key = (io.trial0 + (uint64_t)trial) | ((io.sample0 + (uint64_t)s) << 32);

        auto draw = [&](int64_t t, Vec<4>& z) {
            if (zs) { load_vec<4>(zs + t * 4, z); return; }
            normal_pair(io.seed, key, (uint32_t)(2 * t), kStreamPosterior, z.v[0], z.v[1]);
            normal_pair(io.seed, key, (uint32_t)(2 * t + 1), kStreamPosterior, z.v[2], z.v[3]);
        };
        auto store = [&](int64_t t, const Vec<4>& x) {
            if (px) { CGP_UNROLL for (int i = 0; i < 4; i++) px[t * 4 + i] = x.v[i]; }
            if (pc) pc[t] = sample_fn(io.func, io.comp == 0 ? x.v[0] : io.comp == 1 ? x.v[1] : io.comp == 2 ? x.v[2] : x.v[3]);      // (selects: a run-time index would put x in scratch)
        };

        // the last row: x = mf + L(Pf) z, the pivots against Pf's own diagonal (the same in every lane)
        Vec<4> x;
        {
            Vec<4> mf, z; Sym<4> Pf, L;
            load_vec<4>(mfs + (T - 1) * 4, mf);
            load_sym<4>(Pfs + (T - 1) * 16, Pf);
            cholesky_pivot_rule<4>(Pf, Pf, L);
            draw(T - 1, z);
            CGP_UNROLL for (int i = 0; i < 4; i++) {
                double a = mf.v[i];
                CGP_UNROLL for (int k = 0; k <= i; k++) a = fma(L(i, k), z.v[k], a);
                x.v[i] = a;
            }
            store(T - 1, x);
        }

        // tile j covers the steps T - 2 - 64 j - 63 .. T - 2 - 64 j; lane l of phase G has step base + l (before the record's start: none)
        for (int64_t hi = T - 2; hi >= 0; hi -= 64) {
            const int64_t base = hi - 63;
            wave_lds_fence();                                             // the walk of the tile before has read its records
            {
                const int64_t t = base + lane;
                if (t >= 0) {
                    Vec<4> mf, c; Sym<4> Pf, C, L; Mat<4> G;
                    load_vec<4>(mfs + t * 4, mf);
                    load_sym<4>(Pfs + t * 16, Pf);
                    sample_map(elem, mf, Pf, G, c, C);
                    cholesky_pivot_rule<4>(C, Pf, L);
                    double* mine = recs + lane * kSampRec;
                    CGP_UNROLL for (int a = 0; a < 4; a++) {
                        CGP_UNROLL for (int k = 0; k < 4; k++) mine[kSampG + a * 4 + k] = G.a[a][k];
                        mine[kSampc + a] = c.v[a];
                    }
                    CGP_UNROLL for (int a = 0; a < Sym<4>::N; a++) mine[kSampL + a] = L.a[a];
                }
            }
            wave_lds_fence();
            // the walk: the tile's steps from its last to its first, one compact loop body (a step before the record's start does not exist)
            const int first = base < 0 ? (int)-base : 0;
            _Pragma("unroll 1") for (int k = 63; k >= first; k--) {
                const int64_t t = base + k;
                const double* rec = recs + k * kSampRec;
                Vec<4> z, xn;
                draw(t, z);
                CGP_UNROLL for (int i = 0; i < 4; i++) {
                    double a = rec[kSampc + i];
                    CGP_UNROLL for (int m = 0; m < 4; m++) a = fma(rec[kSampG + i * 4 + m], x.v[m], a);
                    CGP_UNROLL for (int m = 0; m <= i; m++) a = fma(rec[kSampL + Sym<4>::idx(i, m)], z.v[m], a);
                    xn.v[i] = a;
                }
                x = xn;
                store(t, x);
            }
        }
    }
}

template <class Elem>
inline hipError_t launch_sample4(const SampleIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0 || io.S <= 0) return hipSuccess;
    const size_t dyn = Elem::USES_SIGMA ? sigma_lds_bytes(ma, 4) : 0;
    const int64_t groups = (io.S + 63) / 64;
    hipLaunchKernelGGL(sample4_kernel<Elem>, dim3((unsigned)io.B, (unsigned)(groups < 65535 ? groups : 65535)), dim3(64), dyn, stream, io, ma);
    return hipGetLastError();
}

// cgp_inst_sample.hip
int dispatch_sample4(int method, int model_id, const SampleIO& io, const ModelArgs& ma, hipStream_t st);

}  // namespace cgp
