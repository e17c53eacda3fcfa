// cgp_kernels.hpp -- the scan kernels: a forward pass over T measurements (filters) and a reverse pass over the
// filtering results (smoothers), batched over independent trials.  Layouts are the reference's batch-major
// (B, T, ...) arrays (jax.vmap over ys: tetralith/jobs/crlb_ekf.py:68-72).
//
// Launch shapes (block = one 64-lane wavefront in both):
//   WAVE  = true  : grid = B.   One wavefront per trial; ys is fetched 64 steps at a time with one coalesced 512-B
//                   load and handed out by v_readlane; lane 0 streams the 8(d + d^2 + 1) output bytes of each step
//                   (consecutive steps of a trial are contiguous in HBM, so L2 write-combines them into full lines).
//   WAVE  = false : grid = ceil(B / 64).  One lane per trial (large batches).
#pragma once
#include "cgp_steps.hpp"
#ifndef __HIPCC_RTC__          // the context is host code
#include "cgp_ctx.hpp"
#else
struct cgp_ctx;
#endif
#include "../../include/chirpgp_hip.h"

namespace cgp {

struct FilterIO {
    const double* __restrict__ H;  int64_t H_stride;
    const double* __restrict__ Xi; int64_t Xi_stride;
    const double* __restrict__ m0; int64_t m0_stride;
    const double* __restrict__ P0; int64_t P0_stride;
    const double* __restrict__ ys;
    int64_t ys_stride;                       // doubles between records (T for the dense [B][T] layout; 0 = one shared record)
    int64_t ys_repeat;                       // >= 1: consecutive trials served by one record
    const int32_t* __restrict__ ys_index;    // optional record number per group of ys_repeat trials
    int64_t B, T;
    double* __restrict__ mfs;
    double* __restrict__ Pfs;
    double* __restrict__ nll;
    uint32_t flags;
    unsigned long long* __restrict__ counters = nullptr;      // cgp_debug_set(CGP_DBG_COUNT_REGIMES): regime counters of the context, or NULL
    // Time-split filters with burn-in (cgp_filter_time_split; round 4): `segs` wavefronts per trial.  Wavefront (b, s) filters the
    // steps [s seg_len - burn_in, (s + 1) seg_len) of trial b from (m0, P0), writes rows from s seg_len on, and leaves in
    // seg_state[(b segs + s) seg_stride ..] its record (SegRecord below): its state at the junction (after its last burn-in step), its
    // state after its last step and its NLL total.  seg_len and burn_in are multiples of 64 (the kernels' chunk).  segs <= 1: off.
    int segs = 1;
    int64_t seg_len = 0, burn_in = 0;
    double* __restrict__ seg_state = nullptr;
    int seg_stride = 0;
    // The measurement record of a trial (include/chirpgp_hip.h, cgp_filter): trial b reads record ys_index[b / ys_repeat]
    // (b / ys_repeat without an index) -- a parameter sweep or the 2 P + 1 probes of a difference gradient read ONE copy.
    __device__ __forceinline__ const double* record(int64_t trial) const {
        int64_t g = trial;
        if (ys_repeat > 1) g = (int64_t)((uint64_t)trial / (uint64_t)ys_repeat);
        if (ys_index) g = ys_index[g];
        return ys + g * ys_stride;
    }
    // Per-step intervals of a timed call (include/chirpgp_hip_timed.h, cgp_filter_timed): dts[t] is the time from sample t - 1 to sample t,
    // dts[0] from the initial condition to sample 0.  They belong to the record: trial b reads those of the record its measurements come
    // from, dts_stride doubles apart (0: one time grid for the whole call).  NULL on every other call; read by the timed kernels alone.
    // (Behind every older member, so that none of them moves.)
    const double* __restrict__ dts = nullptr;
    int64_t dts_stride = 0;
    __device__ __forceinline__ const double* intervals(int64_t trial) const {
        int64_t g = trial;
        if (ys_repeat > 1) g = (int64_t)((uint64_t)trial / (uint64_t)ys_repeat);
        if (ys_index) g = ys_index[g];
        return dts + g * dts_stride;
    }
};

// The span of time steps of workgroup v of a (possibly time-split) filter launch.
struct FilterSpan {
    int64_t trial, t_begin, t_out, t_end;      // filters [t_begin, t_end), writes rows [t_out, t_end)
    int seg;
    double* state;                             // this segment's record in FilterIO::seg_state, or NULL
};
// SPLIT = false: a kernel instantiated for whole-record launches only -- the span is (0, 0, T) at compile time and everything that
// serves the segments folds away (the sigma-point kernels measured 2 % slower with the run-time form in their default launch).
template <bool SPLIT = true>
__device__ __forceinline__ FilterSpan filter_span(const FilterIO& io, int64_t v) {
    if (!SPLIT || io.segs <= 1) return {v, 0, 0, io.T, 0, nullptr};
    const int64_t b = (int64_t)((uint64_t)v / (uint64_t)io.segs);
    const int s = (int)(v - b * io.segs);
    const int64_t t_out = (int64_t)s * io.seg_len;
    int64_t t_begin = s > 0 ? t_out - io.burn_in : 0;
    if (t_begin < 0) t_begin = 0;
    int64_t t_end = t_out + io.seg_len;
    if (t_end > io.T) t_end = io.T;
    return {b, t_begin, t_out, t_end, s, io.seg_state ? io.seg_state + (b * io.segs + s) * io.seg_stride : nullptr};
}
// The record of one segment, FilterSpan::state: (m, P) at the junction | (m, P) after the last step | NLL total, each (m, P) as d doubles of
// mean and d x d of covariance, row-major.  THE definition: the kernels write through SegRecord<D>, the fix-up pass and the host (whose d
// is a run-time value) read seg_layout(d).
struct SegLayout { int junction, end, nll, stride; };
constexpr SegLayout seg_layout(int d) { return {0, d + d * d, 2 * (d + d * d), 2 * (d + d * d) + 1}; }
template <int D> struct SegRecord {
    static constexpr int kJunction = seg_layout(D).junction, kEnd = seg_layout(D).end, kNll = seg_layout(D).nll, kStride = seg_layout(D).stride;
    // `at` = kJunction or kEnd.  One entry per owning lane: m[i] (the column-form mean of the d = 4 tile layout: lanes 0..3, i = lane) ...
    CGP_DEV static void put_mean(double* rec, int at, bool owner, int i, double mi) { if (owner) rec[at + i] = mi; }
    // ... or the replicated mean of d = 4, from lane 0
    CGP_DEV static void put_mean(double* rec, int at, int lane, double u0, double u1, double u2, double u3) {
        if (lane == 0) { rec[at] = u0; rec[at + 1] = u1; rec[at + 2] = u2; rec[at + 3] = u3; }
    }
    CGP_DEV static void put_cov(double* rec, int at, bool owner, int i, int j, double Pij) { if (owner) rec[at + D + i * D + j] = Pij; }
    CGP_DEV static void put_nll(double* rec, int lane, double total) { if (lane == 0) rec[kNll] = total; }
};
// Junction mismatch of the time-split fix-up passes: max |a - ref| / max |ref| over the d entries of the mean and, apart, the d x d of the
// covariance; inf if a NaN sits on either side.
CGP_DEV double junction_mismatch(const double* am, const double* aP, const double* rm, const double* rP, int d) {
    double dm = 0.0, sm = 0.0, dp = 0.0, sp = 0.0;
    bool nan = false;
    for (int i = 0; i < d; i++) { const double e = fabs(am[i] - rm[i]); nan = nan || !(e == e); dm = fmax(dm, e); sm = fmax(sm, fabs(rm[i])); }
    for (int i = 0; i < d * d; i++) { const double e = fabs(aP[i] - rP[i]); nan = nan || !(e == e); dp = fmax(dp, e); sp = fmax(sp, fabs(rP[i])); }
    const double err = fmax(sm > 0.0 ? dm / sm : dm, sp > 0.0 ? dp / sp : dp);
    return nan ? __builtin_inf() : err;
}

// Selected outputs of a smoother launch (cgp_smoother_select; SURVEY 8f-2: the step right behind the smoother in every driver of the
// reference keeps mss[:, k], Pss[:, k, k] and E[g(V)] of that marginal -- demos/ekfs_mle.py:69-77, quadratures.py:234-274):
// per (trial, step) the smoothed mean and variance of ONE state component and / or E[f(V)], V ~ N(mean, variance), by 1-D
// Gauss-Hermite -- written as [B][T] arrays by the kernel that produced them, so that a pipeline that needs nothing else (mss / Pss
// NULL) writes 8 - 24 bytes a step instead of 8 (d + d^2).
struct SmoothSel {
    int comp = -1;                          // state component; < 0: nothing selected
    int func = 0, order = 0;                // CGP_FN_* integrand and number of nodes of `expect`
    double* __restrict__ mean = nullptr;    // [B][T] or NULL
    double* __restrict__ var = nullptr;     // [B][T] or NULL
    double* __restrict__ expect = nullptr;  // [B][T] or NULL
    const double* __restrict__ xi = nullptr;   // [order] nodes, the reference's scaling (sqrt(2) x the Hermite roots)
    const double* __restrict__ w = nullptr;    // [order] weights, normalised
};
// E[f(m + s Z)] over the rule's nodes: the loop of quadratures.py:218-231 for d = 1.  The softplus integrand (the reference's g,
// models.py:50: the one every driver uses) in three tiers, chosen per LANE so that an element's value does not depend on its neighbours
// in the wavefront (a tier is evaluated by the wavefront only if one of its lanes needs it):
//   1. every node x >= 6 (a frequency above 6 Hz with its whole Gauss-Hermite fan):  log(e^x + 1) = x + log1p(t), t = e^-x <= 2.5e-3, the
//      exponential by the degree-7 near-minimax polynomial of the speculative EKF step (5.5e-11 of t, i.e. 2e-14 of the softplus) and
//      log1p by six terms of its series (truncation t^7 / 7 < 1e-19): ~25 instructions a node;
//   2. any |x| < 700: the branch-free full-accuracy softplus of cgp_fastmath.hpp (softplus_pair_any), ~80 a node;
//   3. otherwise (overflow, inf, NaN) and for the other integrands: the library functions, as cgp_gaussian_expectation_fn evaluates them --
//      but log1p(e^x) at the nodes below 0, where the naive 1 + e^x rounds the softplus away (0 instead of e^x from x = -37 down: a fan that
//      reaches -700 jumped from the second tier's 1e-304 to 0).
CGP_DEV double gh_expectation(int func, double m, double s, const double* __restrict__ xi, const double* __restrict__ w, int order) {
    double fast = 0.0;
    bool have = false;
    if (func == CGP_FN_SOFTPLUS) {
        // the fan's extreme nodes decide the lane's tier before anything is evaluated (NaN: neither)
        double reach = 0.0;
        for (int p = 0; p < order; p++) reach = fmax(reach, fabs(xi[p]));
        reach *= fabs(s);
        const bool tier1 = (m - reach >= 6.0) && (m + reach < 700.0);
        const bool tier2 = !tier1 && (m - reach > -700.0) && (m + reach < 700.0);
        if (__builtin_amdgcn_ballot_w64(tier1) != 0) {
            double acc = 0.0;
            for (int p = 0; p < order; p++) {
                const double x = fma(s, xi[p], m);
                const double t = exp_neg_lean_lit(x);
                double q = kLog1pSeries[0];                                    // log1p(t) / t = 1 - t/2 + t^2/3 - t^3/4 + t^4/5 - t^5/6
                CGP_UNROLL for (int i = 1; i < 6; i++) q = fma(q, t, kLog1pSeries[i]);
                acc = fma(w[p], fma(q, t, x), acc);
            }
            fast = acc;
        }
        if (__builtin_amdgcn_ballot_w64(tier2) != 0) {
            double acc = 0.0;
            for (int p = 0; p < order; p++) {
                const double x = fma(s, xi[p], m);
                double sp, dsp; bool okp;
                softplus_pair_any(x, sp, dsp, okp);
                acc = fma(w[p], sp, acc);
            }
            fast = tier2 ? acc : fast;
        }
        have = tier1 || tier2;
        if (__builtin_amdgcn_ballot_w64(!have) == 0) return fast;
    }
    // (the integrand switch of gaussian_expectation_kernel, cgp_api.hip, written out again: called as a shared function from here, by value
    // or as the whole loop, this function comes out with other branches and registers -- cgp_api and cgp_inst_walk4 differed)
    double acc = 0.0;
    for (int p = 0; p < order; p++) {
        const double x = fma(s, xi[p], m);
        double f;
        if (func == CGP_FN_SOFTPLUS) { const double e = exp(x); f = x < 0.0 ? log1p(e) : log(e + 1.0); }   // models.py:50, the naive form (overflow, NaN as is)
        else if (func == CGP_FN_EXP) f = exp(x);
        else if (func == CGP_FN_SQUARE) f = x * x;
        else f = x;
        acc = fma(w[p], f, acc);
    }
    return have ? fast : acc;
}
// The same as a CALL: the epilogue of the wave-per-trial smoothers runs once per tile, outside their walks -- a call keeps its three
// loops out of kernels that are scheduled around matrix instructions (inlined, hipcc 7.2's "Rewrite AGPR-Copy-MFMA" pass crashed on
// coop8_split_kernel<SgpsElement<LinearDisc<8>>, kWalkApply, true> under -amdgpu-mfma-vgpr-form).
__device__ __attribute__((noinline)) double gh_expectation_call(int func, double m, double s, const double* __restrict__ xi, const double* __restrict__ w, int order) {
    return gh_expectation(func, m, s, xi, w, order);
}
// The rule's nodes and weights staged in LDS once per workgroup (rule[0 .. order) nodes, rule[32 .. 32 + order) weights; order <= 32,
// checked by the C-ABI): read from global memory inside the node loop, every iteration waited for two dependent loads -- the epilogue of
// the lane kernel cost 11 ms per 262 144 x 500 instead of 3.  The caller fences (wave_lds_fence / __syncthreads) before the first use.
constexpr int kGhMaxOrder = 32;
CGP_DEV void sel_stage_rule(const SmoothSel& s, double* rule, int tid) {
    if (s.expect && tid < s.order) { rule[tid] = s.xi[tid]; rule[kGhMaxOrder + tid] = s.w[tid]; }
}
// one (trial, step) of the selected outputs; idx = trial * T + step
CGP_DEV void sel_write(const SmoothSel& s, const double* rule, int64_t idx, double m, double v) {
    if (s.mean) s.mean[idx] = m;
    if (s.var) s.var[idx] = v;
    if (s.expect) s.expect[idx] = gh_expectation_call(s.func, m, sqrt(v), rule, rule + kGhMaxOrder, s.order);
}

struct SmootherIO {
    const double* __restrict__ mfs;
    const double* __restrict__ Pfs;
    int64_t B, T;
    double* __restrict__ mss;
    double* __restrict__ Pss;
    uint32_t flags;
    // time-split discrete smoothers (cgp_walk4.hpp, cgp_coop8.hpp): `segs` wavefronts per trial, each walking `tiles_per_seg`
    // 64-step tiles; the segments' composed maps (A, c, C) live in `ws` between the two passes.  segs <= 1: one wave per trial.
    // (How many: walk_segments, cgp_route.hpp.)  The three sit at byte offsets 52, 64 and 72, where the walks were measured, with the
    // integers of the split with burn-in between them: packed together they shift, and the register allocation of coop8_split_kernel
    // shifts with its arguments' offsets (2 and 6 more AGPR spill slots at d = 6 and d = 8).
    int segs = 1;
    int bsegs = 1, chunks_per_bseg = 0;      // (time-split with burn-in: below)
    int tiles_per_seg = 0;
    int burn_chunks = 0;
    double* __restrict__ ws = nullptr;
    // Time-split with burn-in of the continuous-discrete smoothers (cgp_smoother_time_split; round 6): their backward ODE is not affine in the
    // carry, so a segment cannot be composed exactly -- but the recursion FORGETS its terminal condition like the filters forget their initial
    // one: segment s (0 = the last in time) starts `burn_chunks` 64-step chunks LATER than its piece from the filtering row there, writes
    // nothing until its piece begins, and leaves its state at the junction in junction[(trial * bsegs + s) * kJunctionDoubles] (m 4 | P 16)
    // for the fix-up pass to compare with the row the segment before it wrote.  bsegs <= 1: off.
    static constexpr int kJunctionDoubles = 4 + 16;
    double* __restrict__ junction = nullptr;
    SmoothSel sel;                // cgp_smoother_select: selected outputs (mss / Pss may then be NULL); comp < 0: off
    // Per-step intervals of a timed call (include/chirpgp_hip_timed.h, cgp_smoother_timed): the step from row t + 1 to row t runs over
    // dts[t + 1]; dts[0] is never read.  A smoother has no record addressing of its own, so the intervals bring theirs, with FilterIO::record's
    // rule: trial b reads grid dts_index[b / dts_repeat] (b / dts_repeat without an index), dts_stride doubles apart (0: one grid for the call).
    // NULL on every other call; read by the timed kernels alone.  (Behind every older member, so that none of them moves.)
    const double* __restrict__ dts = nullptr;
    int64_t dts_stride = 0, dts_repeat = 1;
    const int32_t* __restrict__ dts_index = nullptr;
    __device__ __forceinline__ const double* intervals(int64_t trial) const {
        int64_t g = trial;
        if (dts_repeat > 1) g = (int64_t)((uint64_t)trial / (uint64_t)dts_repeat);
        if (dts_index) g = dts_index[g];
        return dts + g * dts_stride;
    }
};
static_assert(__builtin_offsetof(SmootherIO, segs) == 52 && __builtin_offsetof(SmootherIO, tiles_per_seg) == 64 && __builtin_offsetof(SmootherIO, ws) == 72,
              "the walks' arguments moved: compare their register use (tools/resusage.py) before and after");

// ---- the arguments of the other kernel families, next to the filters' and smoothers': the pure half of their entry points (cgp_args.hpp) fills them
// the tangent kernels (cgp_tangent4.hpp, cgp_tangent4_sigma.hpp, cgp_tangent4_cd.hpp)
struct TangentIO {
    const double* __restrict__ H;  int64_t H_stride;
    const double* __restrict__ Xi; int64_t Xi_stride;
    const double* __restrict__ m0; int64_t m0_stride;
    const double* __restrict__ P0; int64_t P0_stride;
    const double* __restrict__ ys; int64_t ys_stride, ys_repeat; const int32_t* __restrict__ ys_index;
    const double* __restrict__ dirs;     // [B][n_dir][kDirDoubles]
    int64_t B, T;
    int n_dir;
    double* __restrict__ nll;            // [B]
    double* __restrict__ grad;           // [B][n_dir]
    double* __restrict__ fisher;         // [B][n_dir][n_dir]: the Fisher forms only (NULL otherwise)
    __device__ __forceinline__ const double* record(int64_t trial) const {
        int64_t g = trial;
        if (ys_repeat > 1) g = (int64_t)((uint64_t)trial / (uint64_t)ys_repeat);
        if (ys_index) g = ys_index[g];
        return ys + g * ys_stride;
    }
};
// LDS the continuous-discrete sigma-point tangent kernel (cgp_tangent4_cd_sigma.hpp) keeps beside the reduction buffer, the direction table and
// the staged set: the RK4 step's base point and accumulators, parked across the fan.  prepare_tangent (cgp_args.hpp) leaves it free.
constexpr int kCdSgpParkBytes = 4608;
// cgp_simulate (cgp_simulate.hpp)
struct SimIO {
    const double* __restrict__ H;  int64_t H_stride;
    const double* __restrict__ Xi; int64_t Xi_stride;
    const double* __restrict__ m0; int64_t m0_stride;
    const double* __restrict__ P0; int64_t P0_stride;
    uint64_t seed;
    int64_t trial0;
    int64_t B, T;
    double* __restrict__ xs;
    double* __restrict__ ys;
    uint32_t vec_ok;       // bit 0: xs rows may be stored as 16-byte chunks, bit 1: ys rows
    uint32_t flags;
};
// cgp_smoother_sample (cgp_sample4.hpp)
struct SampleIO {
    const double* __restrict__ mfs;               // [B][T][4]
    const double* __restrict__ Pfs;               // [B][T][4][4]
    const double* __restrict__ normals;           // [B][S][T][4] or NULL: the Philox stream
    int64_t B, T, S;
    uint64_t seed, trial0, sample0;
    double* __restrict__ paths;                   // [B][S][T][4] or NULL
    double* __restrict__ comp_paths;              // [B][S][T] or NULL
    int comp, func;
};
// cgp_pcrlb_sums (cgp_pcrlb.hpp)
constexpr int kPcrlbSlab = 512;        // trials per workgroup: the atomics stay at 8 K / 512 bytes per trial-step
struct PcrlbIO {
    const double* __restrict__ x0;     // [B][d]
    const double* __restrict__ xs;     // [B][T][d]
    int64_t B, T;
    double* __restrict__ sums;         // [d (d + 1) / 2 + d d][T], accumulated into
};

// Dynamic LDS (sized by the launch): the staged sigma-point set.  The static LDS in front of it (the 17 152-byte
// reduction buffer) is a multiple of 16 bytes, so the base stays 16-byte aligned (cdna_hip_programming.md G17).
CGP_DEV double* dyn_lds() {
    extern __shared__ double cgp_dyn_lds[];
    return cgp_dyn_lds;
}
inline size_t sigma_lds_bytes(const ModelArgs& ma, int d) {
    return ma.sg.xi ? SigmaSet::stage_bytes(ma.sg.s, d, ma.sg.n_groups, ma.sg.group_start != nullptr) : 0;
}
// (the kernels' view of the caller's model and sigma-point set: model_args, cgp_args.hpp)
// The argument structs travel by value, and the run-time-compiled models compare their sizes with this build's after loading (cgp_rtc.hip)
static_assert(sizeof(ModelArgs) == 104 && sizeof(FilterIO) == 208 && sizeof(SmootherIO) == 176, "the kernels' argument structs changed size");

// Linear scalar measurement y = H x + noise (every filter but ekf_for_kpt).
template <int D> struct LinearMeasurement {
    static constexpr bool LINEAR = true;
    CGP_DEV static void update(const Vec<D>& mp, const Sym<D>& Pp, const Vec<D>& H, double Xi, double y, Vec<D>& mf, Sym<D>& Pf,
                               double& S, double& innov, bool skip_missing = false) {
        scalar_update<D>(mp, Pp, H, Xi, y, false, 0.0, mf, Pf, S, innov, skip_missing);
    }
};
// ekf_for_kpt (filters_smoothers.py:298-311): H = grad h(mp), pred = h(mp).
template <int NH, bool UNIFORM = false> struct KptUpdate {
    static constexpr int D = NH + 2;
    static constexpr bool LINEAR = false;
    CGP_DEV static void update(const Vec<D>& mp, const Sym<D>& Pp, const Vec<D>&, double Xi, double y, Vec<D>& mf, Sym<D>& Pf,
                               double& S, double& innov, bool skip_missing = false) {
        Vec<D> H;
        const double pred = KptMeasurement<NH, UNIFORM>::eval(mp, H);
        scalar_update<D>(mp, Pp, H, Xi, y, true, pred, mf, Pf, S, innov, skip_missing);
    }
};

// ---- one-lane-per-trial shape: coalesced rows through LDS -----------------------------------------------------------
// In this shape lane l owns trial (block * 64 + l), and what it reads or writes per step is one ROW of N doubles that is
// contiguous for the trial but T * N doubles away from the neighbouring lane's row.  Issued directly, every 16-byte
// store instruction touches 64 different 128-byte lines (measured: 2.5 TB/s filter, 3.7 TB/s smoother at B = 10^6).
// Instead the 64 rows are transposed through LDS so that consecutive lanes access consecutive 16-byte chunks of the same
// trial's row: each wave instruction then covers whole lines (N = 16: 8 trials x 128 B).  Rows are padded by 16 bytes
// in LDS (pitch N + 2 doubles), which keeps both the row writes and the chunk reads conflict-free.
template <int N> struct RowTile {
    static constexpr int C = N / 2;            // 16-byte chunks per row
    static constexpr int PITCH = N + 2;        // doubles
    static constexpr int DOUBLES = 64 * PITCH;
};

template <int N>
CGP_DEV void block_store_rows(double* tile, int lane, const double (&row)[N], double* __restrict__ out_block,
                              int64_t trial_stride, int nvalid) {
    static_assert(N % 2 == 0, "rows of an even number of doubles");
    using RT = RowTile<N>;
    CGP_UNROLL for (int c = 0; c < RT::C; c++)
        *reinterpret_cast<double2*>(tile + lane * RT::PITCH + 2 * c) = make_double2(row[2 * c], row[2 * c + 1]);
    wave_lds_fence();
    CGP_UNROLL for (int k = 0; k < RT::C; k++) {
        const int g = k * 64 + lane, tr = g / RT::C, ch = g % RT::C;
        const double2 v = *reinterpret_cast<const double2*>(tile + tr * RT::PITCH + 2 * ch);
        if (tr < nvalid) *reinterpret_cast<double2*>(out_block + tr * trial_stride + 2 * ch) = v;
    }
    wave_lds_fence();
}

template <int N>
CGP_DEV void block_load_rows(double* tile, int lane, const double* __restrict__ in_block, int64_t trial_stride, int nvalid,
                             double (&row)[N]) {
    static_assert(N % 2 == 0, "rows of an even number of doubles");
    using RT = RowTile<N>;
    CGP_UNROLL for (int k = 0; k < RT::C; k++) {
        const int g = k * 64 + lane, tr = g / RT::C, ch = g % RT::C;
        const int trc = tr < nvalid ? tr : nvalid - 1;
        const double2 v = *reinterpret_cast<const double2*>(in_block + trc * trial_stride + 2 * ch);
        *reinterpret_cast<double2*>(tile + tr * RT::PITCH + 2 * ch) = v;
    }
    wave_lds_fence();
    CGP_UNROLL for (int c = 0; c < RT::C; c++) {
        const double2 v = *reinterpret_cast<const double2*>(tile + lane * RT::PITCH + 2 * c);
        row[2 * c] = v.x; row[2 * c + 1] = v.y;
    }
    wave_lds_fence();
}

template <int D> CGP_DEV void sym_to_row(const Sym<D>& P, double (&row)[D * D]) {
    CGP_UNROLL for (int i = 0; i < D; i++) CGP_UNROLL for (int j = 0; j < D; j++) row[i * D + j] = P(i, j);
}
template <int D> CGP_DEV void row_to_sym(const double (&row)[D * D], Sym<D>& P) {
    CGP_UNROLL for (int i = 0; i < D; i++) CGP_UNROLL for (int j = 0; j <= i; j++) P(i, j) = row[i * D + j];
}

// ---- one-wave-per-trial shape: a replicated row leaves through LDS -------------------------------------------------------
// Every lane holds the same (mf, Pf); written by lane 0 alone, the d + d^2 doubles of a step are d (d + 1) / 2 16-byte
// store instructions with one active lane each -- 36 for d = 8, 0.9 us of a 4.7 us step (ablation on the C5 filter).
// Instead lane 0 parks the row in LDS (ds_write is cheap with one lane) and lanes 0 .. N/2 - 1 store one 16-byte piece
// each: a single coalesced store instruction per array.
template <int D> struct WaveRow { static constexpr int DOUBLES = D + D * D + ((D + D * D) & 1); };
template <int D>
CGP_DEV void wave_store_step(double* park, int lane, const Vec<D>& m, const Sym<D>& P, double* __restrict__ m_out, double* __restrict__ P_out) {
    if (lane == 0) {
        if constexpr (D % 2 == 0) {
            CGP_UNROLL for (int i = 0; i < D; i += 2) *reinterpret_cast<double2*>(park + i) = make_double2(m.v[i], m.v[i + 1]);
            CGP_UNROLL for (int i = 0; i < D; i++)
                CGP_UNROLL for (int j = 0; j < D; j += 2) *reinterpret_cast<double2*>(park + D + i * D + j) = make_double2(P(i, j), P(i, j + 1));
        } else {
            CGP_UNROLL for (int i = 0; i < D; i++) park[i] = m.v[i];
            CGP_UNROLL for (int i = 0; i < D; i++) CGP_UNROLL for (int j = 0; j < D; j++) park[D + i * D + j] = P(i, j);
        }
    }
    wave_lds_fence();
    if constexpr (D % 2 == 0) {
        CGP_UNROLL for (int base = 0; base < D * D / 2; base += 64) {
            const int c = base + lane;
            if (P_out && c < D * D / 2) *reinterpret_cast<double2*>(P_out + 2 * c) = *reinterpret_cast<const double2*>(park + D + 2 * c);
        }
        if (m_out && lane < D / 2) *reinterpret_cast<double2*>(m_out + 2 * lane) = *reinterpret_cast<const double2*>(park + 2 * lane);
    } else {
        CGP_UNROLL for (int base = 0; base < D * D; base += 64) {
            const int c = base + lane;
            if (P_out && c < D * D) P_out[c] = park[D + c];
        }
        if (m_out && lane < D) m_out[lane] = park[lane];
    }
    wave_lds_fence();
}

// (one lane per trial, EKF at d <= 4: at least two wavefronts per SIMD -- 256 registers; left alone the staged form below takes 371
// and runs one wavefront per SIMD, which leaves its LDS round trips and memory latencies uncovered: 262 144 x 500, full outputs,
// 5.81 -> 5.58 ms, means only 3.15 -> 2.25 ms.  The sigma-point predictions spill under that cap -- 8.6 -> 13.3 ms -- and keep all
// registers: Pred::LANE_TWO_WAVES)
template <class Pred, class Meas>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((!Pred::WAVE && Pred::D <= 4 && Pred::D % 2 == 0 && Pred::LANE_TWO_WAVES) ? 2 : 1)))
filter_kernel(FilterIO io, ModelArgs ma) {
    constexpr int D = Pred::D;
    constexpr bool WAVE = Pred::WAVE;
    constexpr bool TILED = !WAVE && D % 2 == 0;      // one lane per trial: rows go through an LDS transpose
    // ... and, for d = 2 and 4, everything that is NOT a whole 128-byte line per trial and step is STAGED until it is one
    // (round 4, below): measurements and cumulative NLL in groups of 16 steps, filtered means in groups of 16 / d steps
    constexpr bool STAGED = TILED && (D == 2 || D == 4);
    constexpr int kTileDoubles = !TILED ? 1 : (STAGED && RowTile<D * D>::DOUBLES < RowTile<16>::DOUBLES ? RowTile<16>::DOUBLES : RowTile<D * D>::DOUBLES);
    __shared__ double lds[Pred::USES_LDS ? kFanLdsDoubles : 1];
    __shared__ double tile[kTileDoubles];
    __shared__ __attribute__((aligned(16))) double rowpark[WAVE ? WaveRow<D>::DOUBLES : 1];
    constexpr int kYPitch = 17;                      // 16 steps + 1: an odd pitch keeps the per-lane and the per-line accesses conflict-free
    __shared__ double ytile[STAGED ? 64 * kYPitch : 1];
    __shared__ const double* recs[STAGED ? 64 : 1];
    const int lane = threadIdx.x;
    int64_t trial = WAVE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 64 + lane;
    const int64_t block_first = (int64_t)blockIdx.x * 64;
    const int nvalid = (io.B - block_first < 64) ? (int)(io.B - block_first) : 64;      // lane-per-trial shape only
    if constexpr (TILED) {
        // every lane takes part in the cooperative stores: lanes past the batch redo the last trial and store nothing
        if (block_first >= io.B) return;
        if (trial >= io.B) trial = io.B - 1;
    } else {
        if (trial >= io.B) return;
    }

    Pred pred;
    pred.setup(ma, trial);
    if constexpr (Pred::USES_SIGMA && WAVE) pred.sg.stage(dyn_lds(), lane, 64, D);
    Vec<D> H, mf;
    Sym<D> Pf;
    if (io.H) load_vec<D>(io.H + trial * io.H_stride, H);
    else { CGP_UNROLL for (int i = 0; i < D; i++) H.v[i] = 0.0; }
    const double Xi = io.Xi[trial * io.Xi_stride];
    load_vec<D>(io.m0 + trial * io.m0_stride, mf);
    load_sym<D>(io.P0 + trial * io.P0_stride, Pf);

    const int64_t T = io.T;
    const double* __restrict__ ys = io.record(trial);
    // a timed call (cgp_steps.hpp: TimedPredict): the record's intervals, one per step, handed to the predictor before the step
    constexpr bool TIMED = IsTimed<Pred>::value;
    const double* __restrict__ dtr = nullptr;
    if constexpr (TIMED) dtr = io.intervals(trial);
    double* __restrict__ mfs = io.mfs ? io.mfs + trial * T * D : nullptr;
    double* __restrict__ Pfs = io.Pfs ? io.Pfs + trial * T * D * D : nullptr;
    const bool nll_final = (io.flags & CGP_NLL_FINAL_ONLY) != 0;
    double* __restrict__ nll = (io.nll && !nll_final) ? io.nll + trial * T : nullptr;
    const bool writer = !WAVE || lane == 0;
    // CGP_SKIP_MISSING: a NaN measurement leaves the prediction as the step's result (scalar_update) and adds +0.0 to the NLL
    const bool gaps = (io.flags & CGP_SKIP_MISSING) != 0;

    // The negative log-likelihood needs sqrt, log and a divide per step but nothing downstream depends on it, so the
    // wave-per-trial shape keeps it off the serial chain: lane (t mod 64) latches (S, innovation) of step t, and every
    // 64 steps all lanes evaluate their increment at once, prefix-sum it across the wave and store 64 cumulative
    // values with one coalesced 512-B store.
    const bool want_nll = io.nll != nullptr;
    double cum = 0.0, S_l = 1.0, innov_l = 0.0;
    if constexpr (WAVE) {
        for (int64_t t0 = 0; t0 < T; t0 += 64) {
            // 64 measurements with one coalesced 512-B load.  The empty asm consumes the loaded register here, so the
            // compiler's s_waitcnt vmcnt(0) for it sits in this outer loop and not in front of every step's v_readlane
            // (where it would also wait for the previous step's ten output stores to be acknowledged).
            double ychunk = (t0 + lane < T) ? ys[t0 + lane] : 0.0;
            asm volatile("" : "+v"(ychunk));
            double dtchunk = 0.0;                                        // (timed: the chunk's 64 intervals beside its measurements)
            if constexpr (TIMED) {
                dtchunk = (t0 + lane < T) ? dtr[t0 + lane] : 0.0;
                asm volatile("" : "+v"(dtchunk));
            }
            const int nsteps = (T - t0 < 64) ? (int)(T - t0) : 64;
            for (int slot = 0; slot < nsteps; slot++) {
                const int64_t t = t0 + slot;
                const double y = readlane_f64(ychunk, slot);
                Vec<D> mp; Sym<D> Pp;
                double S, innov;
                if constexpr (TIMED) pred.set_interval(readlane_f64(dtchunk, slot));
                pred.predict(lane, lds, mf, Pf, mp, Pp);
                Meas::update(mp, Pp, H, Xi, y, mf, Pf, S, innov, gaps);
                if (lane == slot) { S_l = S; innov_l = innov; }
                if constexpr (D >= 6) {
                    if (mfs || Pfs) wave_store_step<D>(rowpark, lane, mf, Pf, mfs ? mfs + t * D : nullptr, Pfs ? Pfs + t * D * D : nullptr);
                } else if (writer) {      // few enough pieces that the LDS round trip costs more than it saves
                    if (mfs) store_vec<D>(mfs + t * D, mf);
                    if (Pfs) store_sym_full<D>(Pfs + t * D * D, Pf);
                }
            }
            if (want_nll) {
                // (lane l still holds the measurement of step l)
                const bool present = lane < nsteps && !(gaps && is_missing(ychunk));
                double v = (lane < nsteps) ? nll_increment(S_l, innov_l) : 0.0;
                if (gaps) v = present ? v : 0.0;
                v = wave_inclusive_scan(v) + cum;
                if (gaps) v = nll_hold_gaps(v, present, lane, cum);
                if (nll && lane < nsteps) nll[t0 + lane] = v;
                cum = readlane_f64(v, nsteps - 1);
            }
        }
    } else if constexpr (STAGED) {
        // One lane per trial at d = 2 / 4, whole lines only.  Per trial and step the filter reads 8 bytes of measurement and
        // writes 8 bytes of NLL and 8 d bytes of mean -- pieces of 128-byte lines that 64 lanes x several waves per SIMD keep
        // half-filled in L2 for many steps: at 262 144 x 500 (the reference's CRLB job, tetralith/jobs/crlb_ekf.py:59-79) the
        // counters showed 40.9 GB of HBM traffic for 23.1 GB of algorithmic bytes (the measurements fetched seven times over, the
        // means and the NLL written in 32-byte pieces; profiles/r04_ekf_large_*).  So:
        //   * measurements: 64 trials x 16 steps per cooperative load (every load instruction covers four whole lines), parked
        //     in LDS, one ds_read per lane and step; the step's cumulative NLL takes the consumed measurement's slot, and the
        //     tile leaves as whole lines after the 16 steps;
        //   * filtered means: held for 16 / d steps in registers (a lane-uniform select per slot) and stored as ONE 128-byte
        //     row per trial through the same LDS transpose as the covariance rows.
        constexpr int MS = 16 / D;                                   // steps of means per 128-byte line
        recs[lane] = io.record(block_first + (lane < nvalid ? lane : nvalid - 1));
        const int64_t T_lines = T - T % MS;                          // steps whose means leave as whole lines; the rest row by row
        double mh[16];
        CGP_UNROLL for (int i = 0; i < 16; i++) mh[i] = 0.0;
        for (int64_t t0 = 0; t0 < T; t0 += 16) {
            wave_lds_fence();
            _Pragma("unroll 4") for (int k = 0; k < 16; k++) {           // (four loads in flight: more only costs registers)
                const int g = k * 64 + lane, tr = g >> 4, e = g & 15;
                ytile[tr * kYPitch + e] = (t0 + e < T) ? recs[tr][t0 + e] : 0.0;
            }
            wave_lds_fence();
            const int nst = (T - t0 < 16) ? (int)(T - t0) : 16;
            for (int k = 0; k < nst; k++) {
                const int64_t t = t0 + k;
                const double y = ytile[lane * kYPitch + k];
                Vec<D> mp; Sym<D> Pp;
                double S, innov;
                if constexpr (TIMED) pred.set_interval(dtr[t]);            // (the lane's own trial's, clamped like `trial`)
                pred.predict(lane, lds, mf, Pf, mp, Pp);
                Meas::update(mp, Pp, H, Xi, y, mf, Pf, S, innov, gaps);
                if (want_nll) {
                    if (!(gaps && is_missing(y))) cum += nll_increment(S, innov);
                    ytile[lane * kYPitch + k] = cum;
                }
                if (io.mfs) {
                    if (t < T_lines) {
                        const int slot = (int)(t % MS);
                        CGP_UNROLL for (int s = 0; s < MS; s++)
                            CGP_UNROLL for (int i = 0; i < D; i++) mh[s * D + i] = (slot == s) ? mf.v[i] : mh[s * D + i];
                        if (slot == MS - 1) block_store_rows<16>(tile, lane, mh, io.mfs + (block_first * T + (t - (MS - 1))) * D, T * D, nvalid);
                    } else {
                        block_store_rows<D>(tile, lane, mf.v, io.mfs + (block_first * T + t) * D, T * D, nvalid);
                    }
                }
                if (io.Pfs) {
                    double row[D * D];
                    sym_to_row<D>(Pf, row);
                    block_store_rows<D * D>(tile, lane, row, io.Pfs + (block_first * T + t) * D * D, T * D * D, nvalid);
                }
            }
            if (nll) {
                wave_lds_fence();
                _Pragma("unroll 4") for (int k = 0; k < 16; k++) {
                    const int g = k * 64 + lane, tr = g >> 4, e = g & 15;
                    if (tr < nvalid && t0 + e < T) io.nll[(block_first + tr) * T + t0 + e] = ytile[tr * kYPitch + e];
                }
            }
        }
    } else {
        for (int64_t t = 0; t < T; t++) {
            const double y = ys[t];
            Vec<D> mp; Sym<D> Pp;
            double S, innov;
            if constexpr (TIMED) pred.set_interval(dtr[t]);
            pred.predict(lane, lds, mf, Pf, mp, Pp);
            Meas::update(mp, Pp, H, Xi, y, mf, Pf, S, innov, gaps);
            if (want_nll) {
                if (!(gaps && is_missing(y))) cum += nll_increment(S, innov);
                if (nll) nll[t] = cum;
            }
            if constexpr (TILED) {
                if (io.mfs) block_store_rows<D>(tile, lane, mf.v, io.mfs + (block_first * T + t) * D, T * D, nvalid);
                if (io.Pfs) {
                    double row[D * D];
                    sym_to_row<D>(Pf, row);
                    block_store_rows<D * D>(tile, lane, row, io.Pfs + (block_first * T + t) * D * D, T * D * D, nvalid);
                }
            } else {
                if (mfs) store_vec<D>(mfs + t * D, mf);
                if (Pfs) store_sym_full<D>(Pfs + t * D * D, Pf);
            }
        }
    }
    if (writer && io.nll && nll_final) io.nll[trial] = cum;
}

template <class Step>
__global__ void __launch_bounds__(64) smoother_kernel(SmootherIO io, ModelArgs ma) {
    constexpr int D = Step::D;
    constexpr bool WAVE = Step::WAVE;
    constexpr bool TILED = !WAVE && D % 2 == 0;      // one lane per trial: rows go through an LDS transpose
    __shared__ double lds[Step::USES_LDS ? kFanLdsDoubles : 1];
    __shared__ double tile[TILED ? RowTile<D * D>::DOUBLES : 1];
    __shared__ __attribute__((aligned(16))) double rowpark[WAVE ? WaveRow<D>::DOUBLES : 1];
    const int lane = threadIdx.x;
    int64_t trial = WAVE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 64 + lane;
    const int64_t block_first = (int64_t)blockIdx.x * 64;
    const int nvalid = (io.B - block_first < 64) ? (int)(io.B - block_first) : 64;
    if constexpr (TILED) {
        if (block_first >= io.B) return;
        if (trial >= io.B) trial = io.B - 1;
    } else {
        if (trial >= io.B) return;
    }

    Step step;
    step.setup(ma, trial);
    if constexpr (Step::USES_SIGMA && WAVE) step.sg.stage(dyn_lds(), lane, 64, D);
    if constexpr (IsSubstepped<Step>::value) {          // CGP_RK4_SUBSTEPS (cgp_steps.hpp: SubstepSmooth): the interval's intermediate moments
        __shared__ double subtab[SubTable<D>::DOUBLES];
        step.attach(subtab);
    }
    const int64_t T = io.T;
    // a timed call (cgp_steps.hpp: TimedSmooth): the step from row t + 1 to row t runs over dts[t + 1] of the trial's grid
    constexpr bool TIMED = IsTimed<Step>::value;
    const double* __restrict__ dtr = nullptr;
    if constexpr (TIMED) dtr = io.intervals(trial);
    Vec<D> ms, mf;
    Sym<D> Ps, Pf;
    if constexpr (TILED) {
        // filters_smoothers.py:140-142: the last smoothing row is the last filtering row (copied verbatim)
        double row[D * D];
        block_load_rows<D>(tile, lane, io.mfs + (block_first * T + T - 1) * D, T * D, nvalid, ms.v);
        block_store_rows<D>(tile, lane, ms.v, io.mss + (block_first * T + T - 1) * D, T * D, nvalid);
        block_load_rows<D * D>(tile, lane, io.Pfs + (block_first * T + T - 1) * D * D, T * D * D, nvalid, row);
        block_store_rows<D * D>(tile, lane, row, io.Pss + (block_first * T + T - 1) * D * D, T * D * D, nvalid);
        row_to_sym<D>(row, Ps);
        for (int64_t t = T - 2; t >= 0; t--) {
            block_load_rows<D>(tile, lane, io.mfs + (block_first * T + t) * D, T * D, nvalid, mf.v);
            block_load_rows<D * D>(tile, lane, io.Pfs + (block_first * T + t) * D * D, T * D * D, nvalid, row);
            row_to_sym<D>(row, Pf);
            if constexpr (TIMED) step.set_interval(dtr[t + 1]);
            step.step(lane, lds, mf, Pf, ms, Ps);
            block_store_rows<D>(tile, lane, ms.v, io.mss + (block_first * T + t) * D, T * D, nvalid);
            sym_to_row<D>(Ps, row);
            block_store_rows<D * D>(tile, lane, row, io.Pss + (block_first * T + t) * D * D, T * D * D, nvalid);
        }
    } else {
        const double* __restrict__ mfs = io.mfs + trial * T * D;
        const double* __restrict__ Pfs = io.Pfs + trial * T * D * D;
        double* __restrict__ mss = io.mss + trial * T * D;
        double* __restrict__ Pss = io.Pss + trial * T * D * D;
        const bool writer = !WAVE || lane == 0;
        load_vec<D>(mfs + (T - 1) * D, ms);
        load_sym<D>(Pfs + (T - 1) * D * D, Ps);
        if (writer) {   // filters_smoothers.py:140-142: the last smoothing row is the last filtering row (copied verbatim)
            CGP_UNROLL for (int i = 0; i < D; i++) mss[(T - 1) * D + i] = mfs[(T - 1) * D + i];
            CGP_UNROLL for (int i = 0; i < D * D; i++) Pss[(T - 1) * D * D + i] = Pfs[(T - 1) * D * D + i];
        }
        for (int64_t t = T - 2; t >= 0; t--) {
            load_vec<D>(mfs + t * D, mf);
            load_sym<D>(Pfs + t * D * D, Pf);
            if constexpr (TIMED) step.set_interval(dtr[t + 1]);
            step.step(lane, lds, mf, Pf, ms, Ps);
            if constexpr (WAVE && D >= 6) wave_store_step<D>(rowpark, lane, ms, Ps, mss + t * D, Pss + t * D * D);
            else if (writer) {
                store_vec<D>(mss + t * D, ms);
                store_sym_full<D>(Pss + t * D * D, Ps);
            }
        }
    }
}

// Time-parallel discrete smoother (rts / eks / sgp_smoother): one wavefront per trial, K consecutive time steps per
// lane, 64 K steps per tile, tiles walked from the end of the record to its start.  See "TIME-PARALLEL SMOOTHER" in
// cgp_steps.hpp.  Per tile a lane (1) builds the affine maps e_0..e_{K-1} of its steps (the expensive, fully parallel
// part), (2) composes them into one lane aggregate, (3) the 6-round suffix scan runs on the 64 aggregates, (4) the lane
// fetches the composed map of all later lanes, applies it to the carry and then walks its own K steps backwards.
// Cost per 64 steps in wave instructions ~ 734 + 1556 / K (d = 4): K = 4 halves the K = 1 cost.  Loads and stores are
// per-lane runs of K consecutive rows, i.e. one contiguous 64 K * 8 (d + d^2) byte block per tile.
template <class Elem, int K>
__global__ void __launch_bounds__(64) tp_smoother_kernel(SmootherIO io, ModelArgs ma) {
    constexpr int D = Elem::D;
    const int lane = threadIdx.x;
    const int64_t trial = blockIdx.x;
    if (trial >= io.B) return;

    Elem elem;
    elem.setup(ma, trial);
    if constexpr (Elem::USES_SIGMA) elem.sg.stage(dyn_lds(), lane, 64, D);
    const int64_t T = io.T;
    const double* __restrict__ mfs = io.mfs + trial * T * D;
    const double* __restrict__ Pfs = io.Pfs + trial * T * D * D;
    double* __restrict__ mss = io.mss + trial * T * D;
    double* __restrict__ Pss = io.Pss + trial * T * D * D;

    Vec<D> ms;
    Sym<D> Ps;
    load_vec<D>(mfs + (T - 1) * D, ms);
    load_sym<D>(Pfs + (T - 1) * D * D, Ps);
    if (lane == 0) {   // filters_smoothers.py:140-142: last smoothing row = last filtering row, copied verbatim
        CGP_UNROLL for (int i = 0; i < D; i++) mss[(T - 1) * D + i] = mfs[(T - 1) * D + i];
        CGP_UNROLL for (int i = 0; i < D * D; i++) Pss[(T - 1) * D * D + i] = Pfs[(T - 1) * D * D + i];
    }
    for (int64_t hi = T - 2; hi >= 0; hi -= 64 * K) {
        const int64_t base = hi - (64 * K - 1) + (int64_t)lane * K;      // first (earliest) step of this lane
        // all K rows are requested before the first element is built (rows before the start of the record are clamped to
        // row 0 and not used): one memory round trip per tile instead of one per element
        Affine<D> e[K];
        Vec<D> mfk[K]; Sym<D> Pfk[K];
        CGP_UNROLL for (int j = 0; j < K; j++) {
            const int64_t t = base + j >= 0 ? base + j : 0;
            load_vec<D>(mfs + t * D, mfk[j]);
            load_sym<D>(Pfs + t * D * D, Pfk[j]);
        }
        CGP_UNROLL for (int j = 0; j < K; j++) {
            affine_identity<D>(e[j]);
            if (base + j >= 0) elem.element(mfk[j], Pfk[j], e[j]);
        }
        // lane aggregate a = e_0 o e_1 o ... o e_{K-1}
        Affine<D> a = e[K - 1];
        CGP_UNROLL for (int j = K - 2; j >= 0; j--) {
            Affine<D> t = e[j];
            affine_compose<D>(t, a);
            a = t;
        }
        // suffix scan over lanes: a_l <- a_l o a_{l+1} o ... o a_63
        CGP_UNROLL for (int delta = 1; delta < 64; delta *= 2) affine_compose_from_lane<D>(a, delta, lane + delta < 64);
        Vec<D> xm = ms; Sym<D> xP = Ps;
        if constexpr (K == 1) {
            // one step per lane: the scanned map already contains the lane's own step
            affine_apply<D>(a, ms, Ps, xm, xP);
            if (base >= 0) {
                store_vec<D>(mss + base * D, xm);
                store_sym_full<D>(Pss + base * D * D, xP);
            }
        } else {
            // state entering this lane's run from later times: (a_{l+1} o ... o a_63)(carry); lane 63 takes the carry itself
            {
                Affine<D> nxt;
                affine_shfl_down<D>(a, 1, nxt);
                if (lane < 63) affine_apply<D>(nxt, ms, Ps, xm, xP);
            }
            CGP_UNROLL for (int j = K - 1; j >= 0; j--) {
                Vec<D> ym; Sym<D> yP;
                affine_apply<D>(e[j], xm, xP, ym, yP);
                xm = ym; xP = yP;
                if (base + j >= 0) {
                    store_vec<D>(mss + (base + j) * D, xm);
                    store_sym_full<D>(Pss + (base + j) * D * D, xP);
                }
            }
        }
        // carry for the next (earlier) tile: the state at the tile's first step, held by lane 0
        CGP_UNROLL for (int i = 0; i < D; i++) ms.v[i] = readlane_f64(xm.v[i], 0);
        CGP_UNROLL for (int i = 0; i < Sym<D>::N; i++) Ps.a[i] = readlane_f64(xP.a[i], 0);
    }
}

// Steps per lane of the time-parallel smoother: bounded by the VGPR budget (K affine maps of D^2 + D + D(D+1)/2 doubles).
template <int D> struct TpStepsPerLane { static constexpr int value = D <= 4 ? 4 : 1; };

#ifndef __HIPCC_RTC__          // ---- host side: launchers and the dispatch entry points of the translation units
template <class Elem>
inline hipError_t launch_tp_smoother(const SmootherIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return hipSuccess;
    const size_t dyn = Elem::USES_SIGMA ? sigma_lds_bytes(ma, Elem::D) : 0;
    hipLaunchKernelGGL((tp_smoother_kernel<Elem, TpStepsPerLane<Elem::D>::value>), dim3((unsigned)io.B), dim3(64), dyn, stream, io, ma);
    return hipGetLastError();
}

template <class Pred, class Meas>
inline hipError_t launch_filter(const FilterIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return hipSuccess;
    const unsigned grid = Pred::WAVE ? (unsigned)io.B : (unsigned)((io.B + 63) / 64);
    const size_t dyn = (Pred::USES_SIGMA && Pred::WAVE) ? sigma_lds_bytes(ma, Pred::D) : 0;
    hipLaunchKernelGGL((filter_kernel<Pred, Meas>), dim3(grid), dim3(64), dyn, stream, io, ma);
    return hipGetLastError();
}
template <class Step>
inline hipError_t launch_smoother(const SmootherIO& io, const ModelArgs& ma, hipStream_t stream) {
    if (io.B <= 0 || io.T <= 0) return hipSuccess;
    const unsigned grid = Step::WAVE ? (unsigned)io.B : (unsigned)((io.B + 63) / 64);
    const size_t dyn = (Step::USES_SIGMA && Step::WAVE) ? sigma_lds_bytes(ma, Step::D) : 0;
    hipLaunchKernelGGL((smoother_kernel<Step>), dim3(grid), dim3(64), dyn, stream, io, ma);
    return hipGetLastError();
}

// Dispatch tables implemented one per translation unit (cgp_inst_*.hip) so that they compile in parallel: one entry per kernel family
// of cgp_route.hpp, which decides among them.  `key` is d for the linear models and n_harm for the harmonic / KPT ones.  Return
// CGP_E_UNSUPPORTED if the combination is not compiled in (or the launcher's guard refuses it), CGP_E_HIP on a launch error.
int dispatch_filter_disc_linear(int method, int key, bool wave, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_disc_harm(int method, int key, bool wave, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_sde_linear(int method, int key, bool wave, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_sde_harm(int method, int key, bool wave, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_kpt(int key, bool wave, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_kpt8(int key, const FilterIO&, const ModelArgs&, hipStream_t);       // the tile-layout / matrix-core kernels (cgp_kpt8.hpp)
int dispatch_filter_kf4_mfma(const FilterIO&, const ModelArgs&, hipStream_t);            // kf at d = 4 on the matrix cores (cgp_mfma4.hpp)
int dispatch_filter_mfma4(const FilterIO&, const ModelArgs&, hipStream_t);               // ekf, d = 4: one trial or one segment per wavefront
int launch_ekf4_mfma_x4(const FilterIO&, const ModelArgs&, hipStream_t);                 // ... four trials per wavefront
int dispatch_filter_coop4(const FilterIO&, const ModelArgs&, hipStream_t);               // ... on DPP rows (cgp_coop4.hpp)
int dispatch_filter_mfma4_sgp(const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_coop4_sgp(const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_lane4(int method, const FilterIO&, const ModelArgs&, hipStream_t);   // d = 4, one lane per trial, large batches (cgp_lane4.hpp)
int dispatch_filter_coop8_ekf(int n_harm, const FilterIO&, const ModelArgs&, hipStream_t);      // d = 6 / 8 in the 8 x 8 tile layout (cgp_coop8.hpp)
int dispatch_filter_coop8_sgp(int n_harm, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_mfma4_cdekf(const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_coop4_cdekf(const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_mfma4_cdsgp(const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_coop4_cdsgp(const FilterIO&, const ModelArgs&, hipStream_t);
// the one-wavefront-per-trial matrix-core filters for records with gaps (CGP_SKIP_MISSING; cgp_inst_gaps4.hip, cgp_inst_gaps4_sigma.hip)
int dispatch_filter_mfma4_gaps(const FilterIO&, const ModelArgs&, hipStream_t);          // ekf (cgp_inst_gaps4.hip)
int dispatch_filter_mfma4_sgp_gaps(const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_mfma4_cdekf_gaps(const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_mfma4_cdsgp_gaps(const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_disc_linear(int method, int key, bool wave, const SmootherIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_disc_harm(int method, int key, bool wave, const SmootherIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_sde_linear(int method, int key, bool wave, const SmootherIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_sde_harm(int method, int key, bool wave, const SmootherIO&, const ModelArgs&, hipStream_t);
// the same generic kernels with CGP_RK4_SUBSTEPS (cgp_inst_substeps_linear.hip, cgp_inst_substeps_harm.hip); the smoothers one wavefront per trial
int dispatch_filter_sde_linear_substeps(int method, int key, bool wave, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_sde_harm_substeps(int method, int key, bool wave, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_sde_linear_substeps(int method, int key, const SmootherIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_sde_harm_substeps(int method, int key, const SmootherIO&, const ModelArgs&, hipStream_t);
// ... and the one-wavefront-per-trial matrix-core filters at d = 4, with gaps or without (cgp_inst_substeps4.hip)
int dispatch_filter_mfma4_cdekf_substeps(bool gaps, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_mfma4_cdsgp_substeps(bool gaps, const FilterIO&, const ModelArgs&, hipStream_t);
// Timed calls (include/chirpgp_hip_timed.h; cgp_steps.hpp: TimedPredict, TimedSmooth): the generic kernels in both launch shapes, `sub`
// with CGP_RK4_SUBSTEPS -- the smoothers then one wavefront per trial -- (cgp_inst_timed_{linear,harm}_{filters,smoothers}.hip) ...
int dispatch_filter_sde_linear_timed(int method, int key, bool wave, bool sub, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_sde_harm_timed(int method, int key, bool wave, bool sub, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_sde_linear_timed(int method, int key, bool wave, bool sub, const SmootherIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_sde_harm_timed(int method, int key, bool wave, bool sub, const SmootherIO&, const ModelArgs&, hipStream_t);
// ... and the one-wavefront-per-trial matrix-core kernels at d = 4 (cgp_inst_timed4.hip; the smoothers: cgp_inst_timed4_smoothers.hip)
int dispatch_filter_mfma4_cdekf_timed(bool gaps, bool sub, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_filter_mfma4_cdsgp_timed(bool gaps, bool sub, const FilterIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_mfma4_cdeks_timed(const SmootherIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_mfma4_cdsgp_timed(const SmootherIO&, const ModelArgs&, hipStream_t);
// The host side of a smoother launch on the cooperative walks and the large-batch lane kernels: what their launchers need beside the
// kernel's arguments.  Filled from the SmootherDecision (cgp_route.hpp) and the context.
struct WalkSplit { int cap = 1; int min_tiles = 4; };      // exact time split: at most `cap` segments (1: off, 0: as many as fit), of `min_tiles` tiles or more
struct SmootherLaunch {
    cgp_ctx* ctx = nullptr;       // whose per-stream workspace (ctx_workspace) serves SmootherIO::ws
    int num_cus = 256;
    WalkSplit split;
    int lane_buffers = 0;         // cgp_debug_set(CGP_DBG_LANE_BUFFERS): 3 = the large-batch smoothers request their rows two steps ahead, else one
};
int dispatch_smoother_walk4_linear(int method, const SmootherIO&, const SmootherLaunch&, const ModelArgs&, hipStream_t);
int dispatch_smoother_walk4_harm(int method, const SmootherIO&, const SmootherLaunch&, const ModelArgs&, hipStream_t);
int dispatch_smoother_coop8_linear(int method, int d, const SmootherIO&, const SmootherLaunch&, const ModelArgs&, hipStream_t);
int dispatch_smoother_coop8_harm(int method, int n_harm, const SmootherIO&, const SmootherLaunch&, const ModelArgs&, hipStream_t);
int dispatch_smoother_lane4(int method, int model_id, const SmootherIO&, const SmootherLaunch&, const ModelArgs&, hipStream_t);
int dispatch_smoother_mfma4_cdsgp(const SmootherIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_coop4_cdsgp(const SmootherIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_mfma4_cdeks(const SmootherIO&, const ModelArgs&, hipStream_t);
int dispatch_smoother_coop4_cdeks(const SmootherIO&, const ModelArgs&, hipStream_t);

inline int hip_rc(hipError_t e) { return e == hipSuccess ? CGP_OK : CGP_E_HIP; }
// What a dispatch table or a launcher returned, as the C-ABI entry returns it: the two codes a launch ends in get their message
inline int launch_result(cgp_ctx* ctx, int rc) {
    if (rc == CGP_E_UNSUPPORTED) return fail(ctx, rc, "this (method, model, dimension) combination is not compiled in");
    if (rc == CGP_E_HIP) return fail(ctx, rc, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    return rc;
}
// What the pure half of an entry point (prepare_..., cgp_args.hpp) says of a call, and what its enqueue half ends in: a code with the
// message of a refusal (a literal, or text that outlives the call), "nothing to do", or go on -- launch, or go by the code alone.
struct Verdict {
    int rc;
    const char* message;
    bool empty;                   // an empty batch or record: CGP_OK without a launch
    Verdict(int rc_ = CGP_OK, const char* message_ = nullptr, bool empty_ = false) : rc(rc_), message(message_), empty(empty_) {}
};
// The second half of every entry point.  A refusal leaves its message in the context, an empty call is CGP_OK; otherwise enqueue() runs
// on the context's device and its Verdict is what the entry returns: its own message, or launch_result's for its code.  `locked`: under the
// context's launch lock -- one call's launches are enqueued as a unit, since the per-stream scratch of the time-split forms (memset, kernel,
// fix-up) is protected by stream order only if two host threads that share this context AND a stream cannot interleave their launches.
constexpr bool kLaunchLocked = true, kLaunchUnlocked = false;
template <class Enqueue>
inline int launch_on(cgp_ctx* ctx, const Verdict& prepared, bool locked, Enqueue enqueue) {
    if (prepared.rc != CGP_OK) return fail(ctx, prepared.rc, prepared.message ? prepared.message : "");
    if (prepared.empty) return CGP_OK;
    DeviceScope on_device(ctx->device);
    if (!on_device.ok) return fail(ctx, CGP_E_HIP, "hipSetDevice failed");
    std::unique_lock<std::recursive_mutex> launches(ctx->launch_mutex, std::defer_lock);
    if (locked) launches.lock();
    const Verdict done = enqueue();
    return done.message ? fail(ctx, done.rc, done.message) : launch_result(ctx, done.rc);
}
#endif                         // __HIPCC_RTC__

}  // namespace cgp

#include "cgp_route.hpp"       // which of them a call runs, and the admission predicates their launchers guard with
#include "cgp_args.hpp"        // the pure half of every entry point: checks, the route, the launch description
