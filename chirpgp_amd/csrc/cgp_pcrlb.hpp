// cgp_pcrlb.hpp -- Monte-Carlo sums of the posterior Cramer-Rao bound (chirpgp/models.py:583-644, Tichavsky's recursion).
//
// THE MATHEMATICS (the kernel below, the float64 restatement under tests/ and tests/golden/make_exact_pcrlb.py all follow this paragraph).
// Every discrete model here has a Gaussian transition x_t | x_s ~ N(m(x_s), Sigma) with a CONSTANT Sigma, and the measurement
// y = H . x + e, e ~ N(0, Xi), is linear.  For one pair (x_s, x_t) of consecutive states write
//     P = Sigma^-1,    J = dm/dx at x_s,    r = x_t - m(x_s),    w = P r.
// The per-sample blocks of models.py:627-638 are then
//     -d2 log p / dx_s2                         =  J^T P J - sum_i w_i Hess m_i(x_s)      (mean over the trials: D11_t)
//     -d/dx_t grad_{x_s} log p                  = -J^T P        index [s][t], as jacfwd(jacrev(., 1), 0) orders it   (mean: D12_t)
//     -d2 log p / dx_t2 - d2 log p(y | x_t) / dx_t2 = P + H H^T / Xi                      (D22: constant, formed on the host)
// and the recursion is J_t = D22 - D12_t^T (J_{t-1} + D11_t)^-1 D12_t, J_0 = j0, t = 1..T -- not symmetrised, as in the reference.
// The second-order term has zero mean (E[r | x_s] = 0); the reference's Monte-Carlo estimate carries it and so does this one.
//
// CGP_M_LINEAR:  Hess m = 0 and J = F: every entry of both blocks is a constant of the model.
// CGP_M_HARMONIC_LCD (NH harmonics, IV = 2 NH, v = x_s[IV], u = x_s):  with g the softplus, g' = e^v / (1 + e^v), g'' = g' (1 - g'),
//     th_k = (k + 1) dt 2 pi fs g(v),     th_k' = (k + 1) dt 2 pi fs g'(v),     th_k'' = (k + 1) dt 2 pi fs g''(v),
//     (c_k, s_k) = rho (cos, sin)(th_k),  m_2k = c_k u_2k - s_k u_2k+1,  m_2k+1 = s_k u_2k + c_k u_2k+1,  (m_IV, m_IV+1) = M (u_IV, u_IV+1),
//     J = blockdiag(rho Rot(th_k), M) + the column IV:  J[2k][IV] = -th_k' m_2k+1,   J[2k+1][IV] = th_k' m_2k.
// Hess m_i is zero for i >= 2 NH, and for i = 2k, 2k + 1 non-zero only in the entries (2k, IV), (2k+1, IV) (and their transposes) and (IV, IV):
//     Hess m_2k  :  (2k, IV) = -th_k' s_k,   (2k+1, IV) = -th_k' c_k,   (IV, IV) = -th_k'' m_2k+1 - th_k'^2 m_2k
//     Hess m_2k+1:  (2k, IV) =  th_k' c_k,   (2k+1, IV) = -th_k' s_k,   (IV, IV) =  th_k'' m_2k   - th_k'^2 m_2k+1
// Sigma = q I (+) MS, so P = (1/q) I (+) MS^-1 and only the 2 NH + 1 entries of D11 in row IV and the 6 NH entries of D12 in the pair-pair
// blocks and in row IV depend on the sample; the pair-pair blocks of J^T P J are (rho^2 / q) I, the Matern block is M^T MS^-1 M.
//
// THE KERNEL is squared_error_sums_kernel (cgp_api.hip) with a model evaluation in the middle: lane = time step (a wavefront reads 64
// consecutive rows of a trial as one contiguous run), the four wavefronts of a workgroup take every fourth trial of a slab of 512, the
// previous row x_s is the neighbouring lane's x_t (one DPP move per word; lane 0 of a tile loads it, or x0), per-thread accumulators are
// combined through LDS in groups of 8 rows, and wavefront 0 adds one float64 atomic per (row, step) and slab: 8 K / 512 bytes of atomics
// per trial-step against 8 d bytes read.  Only the entries that depend on the sample are summed per trial; an entry that is a constant c
// of the model is added as (trials of the slab) x c.  One more accumulator sums 0 x (every word read), so that a NaN or an infinity in
// xs[b][t] makes ALL rows of steps t and t + 1 NaN and no other step, as a per-sample sum would.
// Sigma^-1 comes from a Cholesky factorisation in IEEE sqrt and division; a pivot <= 0 or NaN (b = 0, say) makes every sum NaN.
// The sums depend on the order in which the slabs' atomics arrive and on how a batch is cut into calls, in their last bits: they are
// NOT reproducible bit for bit from run to run.
#pragma once
#include "cgp_kernels.hpp"

namespace cgp {


constexpr int kPcrlbGroup = 8;         // accumulator rows combined per pass through the LDS buffer

// P = S^-1 of a packed symmetric positive-definite matrix by its Cholesky factor, in IEEE sqrt and division (cgp_math.hpp's cholesky
// trades 5e-15 for speed on a serial chain; this runs once per thread, outside the trial loop).  A pivot <= 0 or NaN makes every entry NaN.
template <int D> CGP_DEV void spd_inverse(const Sym<D>& S, Sym<D>& P) {
    Sym<D> L, W;                       // W = L^-1, lower
    bool bad = false;
    CGP_UNROLL for (int j = 0; j < D; j++) {
        double s = S(j, j);
        CGP_UNROLL for (int k = 0; k < j; k++) s = fma(-L(j, k), L(j, k), s);
        bad = bad || !(s > 0.0);
        L(j, j) = sqrt(s);
        CGP_UNROLL for (int i = j + 1; i < D; i++) {
            double t = S(i, j);
            CGP_UNROLL for (int k = 0; k < j; k++) t = fma(-L(i, k), L(j, k), t);
            L(i, j) = t / L(j, j);
        }
    }
    CGP_UNROLL for (int j = 0; j < D; j++) {
        W(j, j) = 1.0 / L(j, j);
        CGP_UNROLL for (int i = j + 1; i < D; i++) {
            double t = 0.0;
            CGP_UNROLL for (int k = j; k < i; k++) t = fma(-L(i, k), W(k, j), t);
            W(i, j) = t / L(i, i);
        }
    }
    const double poison = bad ? __builtin_nan("") : 0.0;
    CGP_UNROLL for (int i = 0; i < D; i++)
        CGP_UNROLL for (int j = 0; j <= i; j++) {
            double t = 0.0;
            CGP_UNROLL for (int k = i; k < D; k++) t = fma(W(k, i), W(k, j), t);
            P(i, j) = t + poison;
        }
}

// Row numbers of sums: the packed lower triangle of D11 (00 10 11 20 ...), then D12 row-major [s][t]
template <int D> constexpr int pcrlb_row11(int i, int j) { return Sym<D>::idx(i, j); }
template <int D> constexpr int pcrlb_row12(int s, int t) { return Sym<D>::N + s * D + t; }

// What a model contributes: NACC per-thread accumulators (the last one is the NaN carrier), accumulate() per pair, emit() per slab.
template <class DM> struct PcrlbTerms;

// ------------------------------------------------------------------------------------------------ linear: constants only
template <int D_> struct PcrlbTerms<LinearDisc<D_>> {
    static constexpr int D = D_, NACC = 1;
    const double* __restrict__ params;
    CGP_DEV void setup(const ModelArgs& ma) { params = ma.params; }
    CGP_DEV void accumulate(const Vec<D>&, const Vec<D>&, double (&)[NACC]) const {}
    // sums[row][t] += count x constant + carrier, for the slab's `count` trials
    CGP_DEV void emit(const double (&tot)[NACC], double count, double* __restrict__ sums_t, int64_t T) const {
        LinearDisc<D> m;
        m.setup(params, 0.0, 0);
        Sym<D> P;
        spd_inverse<D>(m.Sigma, P);
        Mat<D> A;                                                             // A = F^T P
        CGP_UNROLL for (int s = 0; s < D; s++)
            CGP_UNROLL for (int t = 0; t < D; t++) {
                double a = m.F.a[0][s] * P(0, t);
                CGP_UNROLL for (int i = 1; i < D; i++) a = fma(m.F.a[i][s], P(i, t), a);
                A.a[s][t] = a;
                atomicAdd(sums_t + (int64_t)pcrlb_row12<D>(s, t) * T, fma(count, -a, tot[0]));
            }
        CGP_UNROLL for (int i = 0; i < D; i++)
            CGP_UNROLL for (int j = 0; j <= i; j++) {
                double a = A.a[i][0] * m.F.a[0][j];
                CGP_UNROLL for (int t = 1; t < D; t++) a = fma(A.a[i][t], m.F.a[t][j], a);
                atomicAdd(sums_t + (int64_t)pcrlb_row11<D>(i, j) * T, fma(count, a, tot[0]));
            }
    }
};

// ------------------------------------------------------------------------------------------------ harmonic chirp, LCD
// Accumulators per harmonic k: [6k] sum c_k, [6k+1] sum s_k, [6k+2] sum J[2k][IV], [6k+3] sum J[2k+1][IV] (D12, all times -1/q at the end),
// [6k+4] / [6k+5] the entries (IV, 2k) / (IV, 2k+1) of D11; then [6 NH] the sample's part of D11's (IV, IV) and [6 NH + 1] the NaN carrier.
template <int NH> struct PcrlbTerms<HarmonicLCD<NH>> {
    using DM = HarmonicLCD<NH>;
    static constexpr int D = DM::D, IV = DM::IV, NACC = 6 * NH + 2;
    DM m;
    double pq;                                                                // 1 / q: the pairs' diagonal of Sigma^-1
    Sym<2> PM;                                                                // MS^-1
    CGP_DEV void setup(const ModelArgs& ma) {
        m.setup(ma.params, ma.dt, ma.model_id);
        // Sigma = q I (+) MS block by block: the Cholesky factor of a block-diagonal matrix is its blocks' factors
        Sym<1> Q, PQ;
        Sym<2> MS;
        Q.a[0] = m.q;
        MS(0, 0) = m.MS[0]; MS(1, 0) = m.MS[1]; MS(1, 1) = m.MS[2];
        spd_inverse<1>(Q, PQ);
        spd_inverse<2>(MS, PM);
        pq = PQ.a[0] + 0.0 * PM(0, 0);                                        // a factorisation that breaks anywhere makes every entry NaN
        CGP_UNROLL for (int i = 0; i < 3; i++) PM.a[i] += 0.0 * PQ.a[0];
    }
    CGP_DEV void accumulate(const Vec<D>& u, const Vec<D>& x, double (&acc)[NACC]) const {
        double c[NH], s[NH], jv[2 * NH], hv[2 * NH], hvv;
        m.hessian_contract(u, x, pq, c, s, jv, hv, hvv);
        double jj = 0.0;
        CGP_UNROLL for (int k = 0; k < NH; k++) {
            const double j0 = jv[2 * k], j1 = jv[2 * k + 1];
            acc[6 * k] += c[k];
            acc[6 * k + 1] += s[k];
            acc[6 * k + 2] += j0;
            acc[6 * k + 3] += j1;
            acc[6 * k + 4] += fma(pq, fma(c[k], j0, s[k] * j1), -hv[2 * k]);        // (J^T P J)[2k][IV] = sum_b (rho Rot)[b][0] J[2k+b][IV] / q
            acc[6 * k + 5] += fma(pq, fma(c[k], j1, -(s[k] * j0)), -hv[2 * k + 1]);
            jj = fma(j0, j0, fma(j1, j1, jj));
        }
        acc[6 * NH] += fma(pq, jj, -hvv);
    }
    CGP_DEV void emit(const double (&tot)[NACC], double count, double* __restrict__ sums_t, int64_t T) const {
        const double nan0 = fma(0.0, pq, tot[NACC - 1]);                      // (pq is NaN where a factorisation broke down: the zero entries too)
        // the Matern block: A = M^T MS^-1 (2 x 2), G = A M;  M is row-major in m.M
        double A[2][2], G[2][2];
        CGP_UNROLL for (int a = 0; a < 2; a++)
            CGP_UNROLL for (int b = 0; b < 2; b++) A[a][b] = fma(m.M[a], PM(0, b), m.M[2 + a] * PM(1, b));
        CGP_UNROLL for (int a = 0; a < 2; a++)
            CGP_UNROLL for (int b = 0; b < 2; b++) G[a][b] = fma(A[a][0], m.M[b], A[a][1] * m.M[2 + b]);
        const double rr = (m.rho * m.rho) * pq;
        CGP_UNROLL for (int i = 0; i < D; i++)
            CGP_UNROLL for (int j = 0; j <= i; j++) {
                double v;
                if (i == IV && j < IV) v = tot[6 * (j / 2) + 4 + (j % 2)] + nan0;
                else if (i == IV && j == IV) v = fma(count, G[0][0], tot[6 * NH]) + nan0;
                else if (i > IV) v = (j >= IV) ? fma(count, G[1][j - IV], nan0) : nan0;
                else v = (i == j) ? fma(count, rr, nan0) : nan0;
                atomicAdd(sums_t + (int64_t)pcrlb_row11<D>(i, j) * T, v);
            }
        CGP_UNROLL for (int s = 0; s < D; s++)
            CGP_UNROLL for (int t = 0; t < D; t++) {
                double v = nan0;                                              // -(J^T P)[s][t]
                if (s < IV && t < IV && s / 2 == t / 2) {
                    const int k = s / 2;
                    if (s == t) v = fma(-pq, tot[6 * k], nan0);
                    else v = fma((s < t) ? -pq : pq, tot[6 * k + 1], nan0);   // (rho Rot)[t][s] / q:  [2k][2k+1] = s_k,  [2k+1][2k] = -s_k
                } else if (s == IV && t < IV) v = fma(-pq, tot[6 * (t / 2) + 2 + (t % 2)], nan0);
                else if (s >= IV && t >= IV) v = fma(count, -A[s - IV][t - IV], nan0);
                atomicAdd(sums_t + (int64_t)pcrlb_row12<D>(s, t) * T, v);
            }
    }
};

template <class DM>
__global__ void __launch_bounds__(256) pcrlb_sums_kernel(PcrlbIO io, ModelArgs ma) {
    using Terms = PcrlbTerms<DM>;
    constexpr int D = DM::D, NACC = Terms::NACC, G = kPcrlbGroup;
    __shared__ double part[4][G][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane, T = io.T;
    const int64_t b0 = (int64_t)blockIdx.y * kPcrlbSlab, b1 = (b0 + kPcrlbSlab < io.B) ? b0 + kPcrlbSlab : io.B;
    Terms terms;
    terms.setup(ma);
    double acc[NACC];
    CGP_UNROLL for (int k = 0; k < NACC; k++) acc[k] = 0.0;
    if (t < T) {
        for (int64_t b = b0 + w; b < b1; b += 4) {
            Vec<D> x, u;
            load_vec<D>(io.xs + (b * T + t) * D, x);
            // x_s: the row of the lane below; lane 0 of the tile has none (its own row of the step before, or x0)
            CGP_UNROLL for (int i = 0; i < D; i++) u.v[i] = dpp_zero_f64<0x138, 0xF, 0xF>(x.v[i]);      // wave_shr:1
            if (lane == 0) load_vec<D>(t == 0 ? io.x0 + b * D : io.xs + (b * T + t - 1) * D, u);
            double carrier = 0.0;
            CGP_UNROLL for (int i = 0; i < D; i++) carrier += x.v[i] + u.v[i];
            acc[NACC - 1] = fma(0.0, carrier, acc[NACC - 1]);
            terms.accumulate(u, x, acc);
        }
    }
    double tot[NACC];
    CGP_UNROLL for (int g0 = 0; g0 < NACC; g0 += G) {
        if (g0) __syncthreads();
        CGP_UNROLL for (int k = 0; k < G; k++) if (g0 + k < NACC) part[w][k][lane] = acc[g0 + k];
        __syncthreads();
        CGP_UNROLL for (int k = 0; k < G; k++)
            if (g0 + k < NACC) tot[g0 + k] = (part[0][k][lane] + part[1][k][lane]) + (part[2][k][lane] + part[3][k][lane]);
    }
    if (w == 0 && t < T) terms.emit(tot, (double)(b1 - b0), io.sums + t, T);
}

template <class DM>
inline int launch_pcrlb(const PcrlbIO& io, const ModelArgs& ma, hipStream_t st) {
    const int64_t slabs = (io.B + kPcrlbSlab - 1) / kPcrlbSlab;
    hipLaunchKernelGGL((pcrlb_sums_kernel<DM>), dim3((unsigned)((io.T + 63) / 64), (unsigned)slabs), dim3(256), 0, st, io, ma);
    return hip_rc(hipGetLastError());
}

int dispatch_pcrlb(int model_id, int key, const PcrlbIO&, const ModelArgs&, hipStream_t);

}  // namespace cgp
