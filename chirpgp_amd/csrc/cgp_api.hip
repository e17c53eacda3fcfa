// cgp_api.hip -- the C-ABI of include/chirpgp_hip.h.  Every entry point that launches is three steps: the null-context check, its
// prepare_ function (cgp_args.hpp: argument checks, the route of cgp_route.hpp, the launch description -- nothing is enqueued before
// that verdict) and launch_on (cgp_kernels.hpp) with what it enqueues: workspace, dispatch by route, fix-up and gather launches.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "cgp_kernels.hpp"
#include "../../include/chirpgp_hip_timed.h"
#include "cgp_ctx.hpp"
#include "cgp_sample4.hpp"
#include "cgp_pcrlb.hpp"

namespace cgp {

template <int FN>
__global__ void __launch_bounds__(256) gaussian_expectation_kernel(const double* __restrict__ ms, const double* __restrict__ sd,
                                                                   int64_t n, int64_t stride, const double* __restrict__ xi,
                                                                   const double* __restrict__ w, int order, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double m = ms[i * stride], s = sd[i * stride];
        double acc = 0.0;
        for (int p = 0; p < order; p++) {
            const double x = fma(s, xi[p], m);
            double f;
            if constexpr (FN == CGP_FN_SOFTPLUS) f = log(exp(x) + 1.0);        // models.py:50, the naive form as is
            else if constexpr (FN == CGP_FN_EXP) f = exp(x);
            else if constexpr (FN == CGP_FN_SQUARE) f = x * x;
            else f = x;
            acc = fma(w[p], f, acc);
        }
        out[i] = acc;
    }
}

// cgp_squared_error_sums: lane = time step (64 consecutive steps of a trial are one contiguous 64 d doubles), the four wavefronts of a
// workgroup take every fourth trial of its slab of 512; per-thread sums, then LDS across the wavefronts and one float64 atomic per
// (component, moment, step) and slab.  Reads every byte of a and r once: HBM-bound.
__global__ void __launch_bounds__(256) squared_error_sums_kernel(const double* __restrict__ a, const double* __restrict__ r, int64_t B, int64_t T, int d,
                                                                 ErrComps comps, double* __restrict__ sums) {
    __shared__ double part[4][16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    const int64_t b0 = (int64_t)blockIdx.y * 512, b1 = (b0 + 512 < B) ? b0 + 512 : B;
    double acc[16];
    CGP_UNROLL for (int k = 0; k < 16; k++) acc[k] = 0.0;
    if (t < T) {
        for (int64_t b = b0 + w; b < b1; b += 4) {
            const double* __restrict__ pa = a + (b * T + t) * d;
            const double* __restrict__ pr = r + (b * T + t) * d;
            CGP_UNROLL for (int c = 0; c < 8; c++) {
                if (c < comps.n) {
                    const double e = pa[comps.c[c]] - pr[comps.c[c]], e2 = e * e;
                    acc[2 * c] += e2;
                    acc[2 * c + 1] = fma(e2, e2, acc[2 * c + 1]);
                }
            }
        }
    }
    CGP_UNROLL for (int k = 0; k < 16; k++) part[w][k][lane] = acc[k];
    __syncthreads();
    if (w == 0 && t < T) {
        CGP_UNROLL for (int k = 0; k < 16; k++) {
            if (k < 2 * comps.n) {
                const double v = (part[0][k][lane] + part[1][k][lane]) + (part[2][k][lane] + part[3][k][lane]);
                atomicAdd(sums + (int64_t)k * T + t, v);          // sums[c][m][t], k = 2 c + m
            }
        }
    }
}

// cgp_smoother_select behind a kernel that writes full rows only: the selected marginal read back out of mss / Pss
__global__ void __launch_bounds__(256) smooth_select_kernel(const double* __restrict__ mss, const double* __restrict__ Pss, int64_t n, int d, SmoothSel sel) {
    __shared__ double ghrule[2 * kGhMaxOrder];
    sel_stage_rule(sel, ghrule, threadIdx.x);
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        sel_write(sel, ghrule, i, mss[i * d + sel.comp], Pss[i * d * d + sel.comp * (d + 1)]);
}

// Scales of the debug ops that evaluate a form with its scales folded into the coefficients (ops 14 / 15): neither is a power of two, so a
// coefficient that missed its scale shows.  The test divides them out again (tests/fastmath_points.py holds the same two numbers).
constexpr double kDebugScale = 0.0439822971502571, kDebugDscale = 2.7;

__global__ void __launch_bounds__(256) debug_math_kernel(int op, const double* __restrict__ x, int64_t n,
                                                         double* __restrict__ o0, double* __restrict__ o1) {
    const bool pairs = op == 22 || op == 23 || op == 25;                 // two-argument ops: (x[2 i], x[2 i + 1]) -> o0[i], o1[i]
    const int64_t count = pairs ? n / 2 : n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = pairs ? x[2 * i] : x[i];
        const double v2 = pairs ? x[2 * i + 1] : 0.0;
        double a = 0.0, b = 0.0;
        switch (op) {
        case 0: a = fast_exp(v); break;
        case 1: a = fast_log_ge1(v); break;
        case 2: fast_sincos(v, a, b); break;
        case 3: a = rcp_nr(v); break;
        case 7: softplus_pair_wide(v, a, b); break;
        case 9: a = rcp_nr1(v); break;
        case 10: { bool ok; softplus_pair_any(v, a, b, ok); if (!ok) { a = __builtin_nan(""); b = a; } break; }      // (not ok -> NaN: the caller's fallback)
        case 11: softplus_pair_mid(v, a, b); break;                                                                   // (valid for |v| <= 2)
        // 12 - 15: the softplus of the speculative EKF step as ekf4_mfma_step_spec1 (cgp_mfma4.hpp) writes it, per regime, with th = 0 and kja = 1
        case 12: {                                                                                                    // COMMON, 1.5 <= v < 700
            SpecRegs R; R.init();
            const double t = exp_neg_lean1(R, v);
            const double lin = fma(1.0, v, -0.0);
            double qa;
            softplus_tail_lean(R, t, qa, b);
            a = fma(qa, t, lin);
            break;
        }
        case 13: {                                                                                                    // LOW, -700 < v <= -1.5
            SpecRegs R; R.init();
            const double kja = 1.0, th = 0.0;
            const double t = exp_neg_lean1(R, -v);                                                                    // t = exp(v)
            const double lin = -th;
            double qa, dsp;
            softplus_tail_lean(R, t, qa, dsp);
            a = fma(qa, t, lin);
            b = (kja * t) * dsp;
            break;
        }
        case 14: {                                                                                                    // HIGH, 5 <= v < 700: kDebugScale x, kDebugDscale x
            SpecRegs R; R.init();
            SpecRegsHigh RH; RH.init(kDebugScale, kDebugDscale);
            const double t = exp_neg_high(R, RH, v);
            const double lin = fma(kDebugScale, v, -0.0);
            double qa;
            softplus_tail_high(RH, t, qa, b);
            a = fma(qa, t, lin);
            break;
        }
        case 15: {                                                                                                    // MID, |v| <= 2: kDebugScale x, kDebugDscale x
            SpecRegsMid M; M.init(kDebugScale, kDebugDscale);
            double ga, hj;
            softplus_mid_polys(M, v, ga, hj);
            a = ga + fma(0.5 * kDebugScale, v, -0.0);
            b = fma(v, hj, 0.5 * kDebugDscale);
            break;
        }
        case 18: a = fast_log_ge1_finite(v); break;
        case 19: a = softplus_batch(v); break;
        case 20: softplus_pair_batch(v, a, b); break;
        case 21: fast_sincos_small(v, a, b); break;
        case 22: a = div_nr(v, v2); break;
        case 23: a = div_nr1(v, v2); break;
        case 24: sqrt_rsqrt(v, a, b); break;
        case 25: a = nll_increment(v, v2); break;
        default: softplus_pair(v, a, b); break;
        }
        o0[i] = a;
        if (o1) o1[i] = b;
    }
}

// The wave-uniform variants: one input element per wavefront (all 64 lanes evaluate the same argument).
__global__ void __launch_bounds__(64) debug_math_uniform_kernel(int op, const double* __restrict__ x, int64_t n,
                                                                double* __restrict__ o0, double* __restrict__ o1) {
    FastMathRegs F;
    if (op == 16 || op == 17) F.init();
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const double v = x[i];
        double a, b;
        if (op == 5) softplus_pair_uniform(v, a, b);
        else if (op == 8) { SpecRegs R; R.init(); double q; const double t = exp_neg_lean(R, v); softplus_tail_lean(R, t, q, b); a = fma(q, t, v); }
        else if (op == 16) softplus_pair_uniform(F, v, a, b);
        else if (op == 17) fast_sincos_uniform(F, v, a, b);
        else fast_sincos_uniform(v, a, b);
        if (threadIdx.x == 0) { o0[i] = a; if (o1) o1[i] = b; }
    }
}

// Fix-up pass of a time-split filter launch (one workgroup per trial):
//   * junction_err[b] = the largest relative mismatch, over the junctions of trial b, between the state a segment's burn-in arrived
//     at and the state the segment before it ended with (max |difference| / max |reference|, mean and covariance separately) --
//     everything the segment wrote afterwards is at most this far from the sequential filter's rows (the filter forgets its
//     initial condition; the caller decides what mismatch it accepts);
//   * the cumulative NLL of segment s > 0 starts at 0: add the totals of the segments before it (or, NLL-final mode, sum the totals).
__global__ void __launch_bounds__(64) filter_split_fixup_kernel(FilterIO io, int d, double* __restrict__ junction_err) {
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const SegLayout L = seg_layout(d);
    const double* __restrict__ rec = io.seg_state + b * io.segs * io.seg_stride;
    double worst = 0.0;
    for (int s = 1; s < io.segs; s++) {
        const double* start = rec + s * io.seg_stride + L.junction;      // (m, P) after the burn-in of segment s
        const double* end = rec + (s - 1) * io.seg_stride + L.end;       // (m, P) after the last step of segment s - 1
        // (a NaN on either side of a junction: the split run is not the sequential one)
        worst = fmax(worst, junction_mismatch(start, start + d, end, end + d, d));
    }
    if (lane == 0) junction_err[b] = worst;
    if (!io.nll) return;
    if (io.flags & CGP_NLL_FINAL_ONLY) {
        if (lane == 0) { double sum = 0.0; for (int s = 0; s < io.segs; s++) sum += rec[s * io.seg_stride + L.nll]; io.nll[b] = sum; }
        return;
    }
    double offset = 0.0;
    for (int s = 1; s < io.segs; s++) {
        offset += rec[(s - 1) * io.seg_stride + L.nll];
        const int64_t t0 = (int64_t)s * io.seg_len, t1 = (t0 + io.seg_len < io.T) ? t0 + io.seg_len : io.T;
        for (int64_t t = t0 + lane; t < t1; t += 64) io.nll[b * io.T + t] += offset;
    }
}

// Fix-up pass of a time-split smoother launch (one wavefront per trial): junction_err[b] = the largest mismatch, over the junctions of trial b,
// between the state a segment's burn-in arrived at and the row the segment before it (later in time) wrote there.  A heuristic like the filters'
// (include/chirpgp_hip.h).
__global__ void __launch_bounds__(64) smoother_split_fixup_kernel(SmootherIO io, double* __restrict__ junction_err) {
    const int64_t trial = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int64_t T = io.T;
    double worst = 0.0;
    for (int s = 1; s < io.bsegs; s++) {
        const int64_t j_own = (int64_t)s * io.chunks_per_bseg;
        if (j_own >= (T - 1 + 63) / 64) break;
        const int64_t row = T - 1 - 64 * j_own;                          // the row both sides hold: segment s - 1 wrote it, segment s arrived at it
        const double* __restrict__ jn = io.junction + (trial * io.bsegs + s) * SmootherIO::kJunctionDoubles;
        worst = fmax(worst, junction_mismatch(jn, jn + 4, io.mss + (trial * T + row) * 4, io.Pss + (trial * T + row) * 16, 4));
    }
    junction_err[trial] = worst;
}

}  // namespace cgp

using namespace cgp;

extern "C" {

int cgp_version(void) { return CGP_VERSION; }

int cgp_create(cgp_ctx** out, int device) {
    if (!out) return CGP_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return CGP_E_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return CGP_E_HIP;
    cgp_ctx* c = new cgp_ctx;
    c->device = device;
    c->num_cus = prop.multiProcessorCount;
    *out = c;
    return CGP_OK;
}

void cgp_destroy(cgp_ctx* ctx) {
    if (!ctx) return;
    {
        DeviceScope on_device(ctx->device);
        if (ctx->counters_mem) (void)hipFree(ctx->counters_mem);
        for (auto& kv : ctx->ws) if (kv.second.p) (void)hipFree(kv.second.p);      // hipFree waits for the device: no launch still uses them
    }
    delete ctx;
}

int cgp_reserve_workspace(cgp_ctx* ctx, size_t bytes, void* stream) {
    if (!ctx) return CGP_E_ARG;
    if (bytes == 0) return CGP_OK;
    DeviceScope on_device(ctx->device);
    if (!on_device.ok) return fail(ctx, CGP_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::recursive_mutex> launches(ctx->launch_mutex);
    if (!ctx_workspace(ctx, (hipStream_t)stream, bytes, /*reserve=*/true)) return fail(ctx, CGP_E_HIP, "workspace allocation failed");
    return CGP_OK;
}

int cgp_release_workspace(cgp_ctx* ctx, void* stream) {
    if (!ctx) return CGP_E_ARG;
    DeviceScope on_device(ctx->device);
    if (!on_device.ok) return fail(ctx, CGP_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::recursive_mutex> launches(ctx->launch_mutex);
    std::lock_guard<std::mutex> lock(ctx->ws_mutex);
    auto it = ctx->ws.find((hipStream_t)stream);
    if (it == ctx->ws.end()) return CGP_OK;
    if (it->second.p) {
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, CGP_E_HIP, "hipStreamSynchronize failed (is the stream being captured?)"); }
        (void)hipFree(it->second.p);
    }
    ctx->ws.erase(it);
    return CGP_OK;
}

const char* cgp_source_hash(void) {
    return
#include "cgp_source_hash.inc"
    ;
}

int cgp_debug_set(cgp_ctx* ctx, int key, int64_t value) {
    if (!ctx) return CGP_E_ARG;
    switch (key) {
    case CGP_DBG_WALK_SEGMENTS:
        if (value < 0 || value > 4096) return fail(ctx, CGP_E_ARG, "CGP_DBG_WALK_SEGMENTS outside 0..4096");
        ctx->walk_segments = (int)value;
        return CGP_OK;
    case CGP_DBG_LANE_BUFFERS:
        if (value != 0 && value != 2 && value != 3) return fail(ctx, CGP_E_ARG, "CGP_DBG_LANE_BUFFERS: 0 (default), 2 or 3");
        ctx->lane_buffers = (int)value;
        return CGP_OK;
    case CGP_DBG_COUNT_REGIMES: {
        if (value != 0 && !ctx->counters_mem) {
            DeviceScope on_device(ctx->device);
            if (!on_device.ok) return fail(ctx, CGP_E_HIP, "hipSetDevice failed");
            if (hipMalloc(&ctx->counters_mem, 8 * sizeof(unsigned long long)) != hipSuccess) return fail(ctx, CGP_E_HIP, "hipMalloc of the counters failed");
            if (hipMemset(ctx->counters_mem, 0, 8 * sizeof(unsigned long long)) != hipSuccess) return fail(ctx, CGP_E_HIP, "hipMemset of the counters failed");
        }
        ctx->counters = value != 0 ? ctx->counters_mem : nullptr;
        return CGP_OK;
    }
    default: return fail(ctx, CGP_E_ARG, "unknown cgp_debug_set key");
    }
}

int cgp_debug_counters(cgp_ctx* ctx, uint64_t* out, int reset, void* stream) {
    if (!ctx) return CGP_E_ARG;
    if (!out) return fail(ctx, CGP_E_ARG, "out is NULL");
    for (int i = 0; i < 8; i++) out[i] = 0;
    if (!ctx->counters_mem) return CGP_OK;
    DeviceScope on_device(ctx->device);
    if (!on_device.ok) return fail(ctx, CGP_E_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(out, ctx->counters_mem, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess) return fail(ctx, CGP_E_HIP, "copy of the counters failed");
    if (reset && hipMemsetAsync(ctx->counters_mem, 0, 8 * sizeof(uint64_t), st) != hipSuccess) return fail(ctx, CGP_E_HIP, "reset of the counters failed");
    if (hipStreamSynchronize(st) != hipSuccess) return fail(ctx, CGP_E_HIP, "hipStreamSynchronize failed");
    return CGP_OK;
}

const char* cgp_last_error(const cgp_ctx* ctx) {
    if (!ctx) return "null context";
    const ThreadError& e = thread_error();
    return e.ctx == ctx ? e.msg.c_str() : "";
}

}  // extern "C"

// The enqueue half of cgp_filter / cgp_filter_time_split: the workspace of the segment records and its NaN fill, the routed kernel, the
// fix-up pass (or, where nothing was split, a junction_err of zeros).
static Verdict enqueue_filter(cgp_ctx* ctx, const FilterCall& c, FilterPlan& p, hipStream_t st) {
    FilterIO& io = p.io;
    const ModelArgs& ma = p.ma;
    const FilterDecision& route = p.route;
    const cgp_model* model = c.model;
    if (io.segs > 1) {
        const size_t seg_doubles = (size_t)io.seg_stride * (size_t)io.B * (size_t)io.segs;
        double* seg_ws = (double*)ctx_workspace(ctx, st, sizeof(double) * seg_doubles);
        if (!seg_ws) return {CGP_E_HIP, "no workspace for the segment records (allocation failed, or the buffer would grow inside a graph capture: cgp_reserve_workspace first)"};
        // NaN-filled: a kernel that ignored the segments would show as junction_err = inf, not as garbage
        if (hipMemsetAsync(seg_ws, 0xFF, sizeof(double) * seg_doubles, st) != hipSuccess) return {CGP_E_HIP, "hipMemsetAsync of the segment records failed"};
        io.seg_state = seg_ws;
    }
    int rc = CGP_OK;
    switch (route.route) {
    case FilterRoute::kGenericWave:
    case FilterRoute::kGenericLane:
        switch (model->model_id) {
        case CGP_M_LINEAR:       rc = dispatch_filter_disc_linear(c.method, model->d, route.wave, io, ma, st); break;
        case CGP_M_HARMONIC_LCD:
        case CGP_M_LASCALA_LCD:  rc = dispatch_filter_disc_harm(c.method, model->n_harm, route.wave, io, ma, st); break;
        case CGP_M_LINEAR_SDE:   rc = route.timed ? dispatch_filter_sde_linear_timed(c.method, model->d, route.wave, route.substeps, io, ma, st)
                                      : route.substeps ? dispatch_filter_sde_linear_substeps(c.method, model->d, route.wave, io, ma, st)
                                                     : dispatch_filter_sde_linear(c.method, model->d, route.wave, io, ma, st); break;
        case CGP_M_HARMONIC_SDE: rc = route.timed ? dispatch_filter_sde_harm_timed(c.method, model->n_harm, route.wave, route.substeps, io, ma, st)
                                      : route.substeps ? dispatch_filter_sde_harm_substeps(c.method, model->n_harm, route.wave, io, ma, st)
                                                     : dispatch_filter_sde_harm(c.method, model->n_harm, route.wave, io, ma, st); break;
        default: rc = CGP_E_ARG;
        }
        break;
    case FilterRoute::kKf4Mfma:     rc = dispatch_filter_kf4_mfma(io, ma, st); break;
    case FilterRoute::kEkf4Mfma:
    case FilterRoute::kEkf4MfmaSeg: rc = route.gaps ? dispatch_filter_mfma4_gaps(io, ma, st) : dispatch_filter_mfma4(io, ma, st); break;
    case FilterRoute::kEkf4MfmaX4:  rc = launch_ekf4_mfma_x4(io, ma, st); break;
    case FilterRoute::kEkf4Coop:    rc = dispatch_filter_coop4(io, ma, st); break;
    case FilterRoute::kSgp4Mfma:    rc = route.gaps ? dispatch_filter_mfma4_sgp_gaps(io, ma, st) : dispatch_filter_mfma4_sgp(io, ma, st); break;
    case FilterRoute::kSgp4Coop:    rc = dispatch_filter_coop4_sgp(io, ma, st); break;
    case FilterRoute::kLane4Ekf:
    case FilterRoute::kLane4Sgp:    rc = dispatch_filter_lane4(c.method, io, ma, st); break;
    case FilterRoute::kEkf8Coop:    rc = dispatch_filter_coop8_ekf(model->n_harm, io, ma, st); break;
    case FilterRoute::kSgp8Coop:    rc = dispatch_filter_coop8_sgp(model->n_harm, io, ma, st); break;
    case FilterRoute::kCdEkf4Mfma:  rc = route.timed ? dispatch_filter_mfma4_cdekf_timed(route.gaps, route.substeps, io, ma, st)
                                         : route.substeps ? dispatch_filter_mfma4_cdekf_substeps(route.gaps, io, ma, st)
                                         : route.gaps ? dispatch_filter_mfma4_cdekf_gaps(io, ma, st) : dispatch_filter_mfma4_cdekf(io, ma, st); break;
    case FilterRoute::kCdEkf4Coop:  rc = dispatch_filter_coop4_cdekf(io, ma, st); break;
    case FilterRoute::kCdSgp4Mfma:  rc = route.timed ? dispatch_filter_mfma4_cdsgp_timed(route.gaps, route.substeps, io, ma, st)
                                         : route.substeps ? dispatch_filter_mfma4_cdsgp_substeps(route.gaps, io, ma, st)
                                         : route.gaps ? dispatch_filter_mfma4_cdsgp_gaps(io, ma, st) : dispatch_filter_mfma4_cdsgp(io, ma, st); break;
    case FilterRoute::kCdSgp4Coop:  rc = dispatch_filter_coop4_cdsgp(io, ma, st); break;
    case FilterRoute::kKpt8Coop:    rc = dispatch_filter_kpt8(model->n_harm, io, ma, st); break;
    case FilterRoute::kGenericKpt:  rc = dispatch_filter_kpt(model->n_harm, route.wave, io, ma, st); break;
    }
    if (rc == CGP_OK && c.junction_err) {
        if (io.segs > 1) {
            hipLaunchKernelGGL(filter_split_fixup_kernel, dim3((unsigned)io.B), dim3(64), 0, st, io, model->d, c.junction_err);
            rc = hip_rc(hipGetLastError());
        } else rc = hip_rc(hipMemsetAsync(c.junction_err, 0, sizeof(double) * (size_t)io.B, st));      // nothing was split: no junction, no mismatch
    }
    return rc;
}

// The enqueue half of cgp_smoother / cgp_smoother_select / cgp_smoother_time_split: the workspace of the junction states, the routed kernel,
// the fix-up pass (or a junction_err of zeros), the gather launch of selected outputs.
static Verdict enqueue_smoother(cgp_ctx* ctx, const SmootherCall& c, SmootherPlan& p, hipStream_t st) {
    SmootherIO& io = p.io;
    const ModelArgs& ma = p.ma;
    const SmootherDecision& plan = p.route;
    const cgp_model* model = c.model;
    const int method = c.method;
    const bool wave = plan.wave;
    const SmootherLaunch host{ctx, ctx->num_cus, plan.split, ctx->lane_buffers};
    if (plan.bsegs > 1) {
        io.junction = (double*)ctx_workspace(ctx, st, sizeof(double) * SmootherIO::kJunctionDoubles * (size_t)io.B * (size_t)plan.bsegs);
        if (!io.junction) return {CGP_E_HIP, "no workspace for the junction states (allocation failed, or the buffer would grow inside a graph capture: cgp_reserve_workspace first)"};
    }
    int rc = CGP_OK;
    switch (plan.route) {
    case SmootherRoute::kCoop8Linear: rc = dispatch_smoother_coop8_linear(method, model->d, io, host, ma, st); break;
    case SmootherRoute::kWalk4Linear: rc = dispatch_smoother_walk4_linear(method, io, host, ma, st); break;
    case SmootherRoute::kDiscLinear:  rc = dispatch_smoother_disc_linear(method, model->d, wave, io, ma, st); break;
    case SmootherRoute::kCoop8Harm:   rc = dispatch_smoother_coop8_harm(method, model->n_harm, io, host, ma, st); break;
    case SmootherRoute::kWalk4Harm:   rc = dispatch_smoother_walk4_harm(method, io, host, ma, st); break;
    case SmootherRoute::kLane4:       rc = dispatch_smoother_lane4(method, model->model_id, io, host, ma, st); break;
    case SmootherRoute::kDiscHarm:    rc = dispatch_smoother_disc_harm(method, model->n_harm, wave, io, ma, st); break;
    case SmootherRoute::kSdeLinear:   rc = plan.timed ? dispatch_smoother_sde_linear_timed(method, model->d, wave, plan.substeps, io, ma, st)
                                           : plan.substeps ? dispatch_smoother_sde_linear_substeps(method, model->d, io, ma, st)
                                                         : dispatch_smoother_sde_linear(method, model->d, wave, io, ma, st); break;
    case SmootherRoute::kCdSgp4Mfma:  rc = plan.timed ? dispatch_smoother_mfma4_cdsgp_timed(io, ma, st) : dispatch_smoother_mfma4_cdsgp(io, ma, st); break;
    case SmootherRoute::kCdSgp4Coop:  rc = dispatch_smoother_coop4_cdsgp(io, ma, st); break;
    case SmootherRoute::kCdEks4Mfma:  rc = plan.timed ? dispatch_smoother_mfma4_cdeks_timed(io, ma, st) : dispatch_smoother_mfma4_cdeks(io, ma, st); break;
    case SmootherRoute::kCdEks4Coop:  rc = dispatch_smoother_coop4_cdeks(io, ma, st); break;
    case SmootherRoute::kSdeHarm:     rc = plan.timed ? dispatch_smoother_sde_harm_timed(method, model->n_harm, wave, plan.substeps, io, ma, st)
                                           : plan.substeps ? dispatch_smoother_sde_harm_substeps(method, model->n_harm, io, ma, st)
                                                         : dispatch_smoother_sde_harm(method, model->n_harm, wave, io, ma, st); break;
    case SmootherRoute::kNone:        rc = CGP_E_ARG; break;
    }
    if (rc == CGP_OK && c.junction_err) {
        if (io.bsegs > 1) {
            hipLaunchKernelGGL(smoother_split_fixup_kernel, dim3((unsigned)io.B), dim3(64), 0, st, io, c.junction_err);
            rc = hip_rc(hipGetLastError());
        } else rc = hip_rc(hipMemsetAsync(c.junction_err, 0, sizeof(double) * (size_t)io.B, st));      // nothing was split: no junction, no mismatch
    }
    if (rc == CGP_OK && plan.select == SmootherSelect::kGather) {
        const int64_t n = io.B * io.T, blocks = (n + 255) / 256;
        hipLaunchKernelGGL(smooth_select_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, io.mss, io.Pss, n, model->d, p.sel);
        rc = hip_rc(hipGetLastError());
    }
    return rc;
}

static int filter_entry(cgp_ctx* ctx, const FilterCall& call, void* stream) {
    if (!ctx) return CGP_E_ARG;
    FilterPlan plan;
    const Verdict prepared = prepare_filter(call, host_of(ctx), plan);
    return launch_on(ctx, prepared, kLaunchLocked, [&]() -> Verdict { return enqueue_filter(ctx, call, plan, (hipStream_t)stream); });
}
static int smoother_entry(cgp_ctx* ctx, const SmootherCall& call, void* stream) {
    if (!ctx) return CGP_E_ARG;
    SmootherPlan plan;
    const Verdict prepared = prepare_smoother(call, host_of(ctx), plan);
    return launch_on(ctx, prepared, kLaunchLocked, [&]() -> Verdict { return enqueue_smoother(ctx, call, plan, (hipStream_t)stream); });
}
// cgp_smoother and cgp_smoother_time_split write full rows: a cgp_smooth_out with nothing selected
static cgp_smooth_out full_rows(double* mss, double* Pss) {
    cgp_smooth_out out;
    memset(&out, 0, sizeof(out));
    out.mss = mss; out.Pss = Pss; out.comp = -1;
    return out;
}

extern "C" {

int cgp_filter(cgp_ctx* ctx, int method, const cgp_model* model, const cgp_sigma* sigma, const cgp_init* init,
               double dt, const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index,
               int64_t B, int64_t T, double* mfs, double* Pfs, double* nll, uint32_t flags, void* stream) {
    return filter_entry(ctx, {method, model, sigma, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T, mfs, Pfs, nll, flags}, stream);
}

int cgp_filter_time_split(cgp_ctx* ctx, int method, const cgp_model* model, const cgp_sigma* sigma, const cgp_init* init,
                          double dt, const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index,
                          int64_t B, int64_t T, double* mfs, double* Pfs, double* nll, uint32_t flags,
                          int64_t segments, int64_t burn_in, double* junction_err, void* stream) {
    return filter_entry(ctx, {method, model, sigma, init, dt, ys, ys_stride, ys_repeat, ys_index, B, T, mfs, Pfs, nll, flags, true, segments, burn_in, junction_err},
                        stream);
}

int cgp_smoother(cgp_ctx* ctx, int method, const cgp_model* model, const cgp_sigma* sigma, double dt,
                 const double* mfs, const double* Pfs, int64_t B, int64_t T, double* mss, double* Pss,
                 uint32_t flags, void* stream) {
    const cgp_smooth_out out = full_rows(mss, Pss);
    return smoother_entry(ctx, {method, model, sigma, dt, mfs, Pfs, B, T, &out, flags}, stream);
}

int cgp_smoother_time_split(cgp_ctx* ctx, int method, const cgp_model* model, const cgp_sigma* sigma, double dt,
                            const double* mfs, const double* Pfs, int64_t B, int64_t T, double* mss, double* Pss,
                            uint32_t flags, int64_t segments, int64_t burn_in, double* junction_err, void* stream) {
    const cgp_smooth_out out = full_rows(mss, Pss);
    return smoother_entry(ctx, {method, model, sigma, dt, mfs, Pfs, B, T, &out, flags, true, segments, burn_in, junction_err}, stream);
}

int cgp_smoother_select(cgp_ctx* ctx, int method, const cgp_model* model, const cgp_sigma* sigma, double dt,
                        const double* mfs, const double* Pfs, int64_t B, int64_t T, const cgp_smooth_out* out,
                        uint32_t flags, void* stream) {
    return smoother_entry(ctx, {method, model, sigma, dt, mfs, Pfs, B, T, out, flags}, stream);
}

// ---- include/chirpgp_hip_timed.h: one interval per step; the kernels read FilterIO::dts / SmootherIO::dts, never ModelArgs::dt
int cgp_filter_timed(cgp_ctx* ctx, int method, const cgp_model* model, const cgp_sigma* sigma, const cgp_init* init,
                     const double* dts, int64_t dts_stride, const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index,
                     int64_t B, int64_t T, double* mfs, double* Pfs, double* nll, uint32_t flags, void* stream) {
    FilterCall call{method, model, sigma, init, 0.0, ys, ys_stride, ys_repeat, ys_index, B, T, mfs, Pfs, nll, flags};
    call.dts = dts; call.dts_stride = dts_stride; call.timed = true;
    return filter_entry(ctx, call, stream);
}

int cgp_smoother_timed(cgp_ctx* ctx, int method, const cgp_model* model, const cgp_sigma* sigma,
                       const double* dts, int64_t dts_stride, int64_t dts_repeat, const int32_t* dts_index,
                       const double* mfs, const double* Pfs, int64_t B, int64_t T, const cgp_smooth_out* out, uint32_t flags, void* stream) {
    SmootherCall call{method, model, sigma, 0.0, mfs, Pfs, B, T, out, flags};
    call.dts = dts; call.dts_stride = dts_stride; call.dts_repeat = dts_repeat; call.dts_index = dts_index; call.timed = true;
    return smoother_entry(ctx, call, stream);
}

int cgp_smoother_sample(cgp_ctx* ctx, int method, const cgp_model* model, const cgp_sigma* sigma, double dt,
                        const double* mfs, const double* Pfs, int64_t B, int64_t T, int64_t S,
                        uint64_t seed, int64_t trial0, int64_t sample0, const double* normals,
                        const cgp_sample_out* out, uint32_t flags, void* stream) {
    if (!ctx) return CGP_E_ARG;
    SampleIO io{};
    ModelArgs ma;
    const Verdict prepared = prepare_smoother_sample(method, model, sigma, dt, mfs, Pfs, B, T, S, seed, trial0, sample0, normals, out, flags, io, ma);
    return launch_on(ctx, prepared, kLaunchLocked, [&]() -> Verdict { return dispatch_sample4(method, model->model_id, io, ma, (hipStream_t)stream); });
}

int cgp_gaussian_expectation(cgp_ctx* ctx, const double* ms, const double* sd, int64_t n, int64_t in_stride,
                             const double* xi, const double* w, int32_t order, double* out, void* stream) {
    return cgp_gaussian_expectation_fn(ctx, CGP_FN_SOFTPLUS, ms, sd, n, in_stride, xi, w, order, out, stream);
}

int cgp_gaussian_expectation_fn(cgp_ctx* ctx, int func, const double* ms, const double* sd, int64_t n, int64_t in_stride,
                                const double* xi, const double* w, int32_t order, double* out, void* stream) {
    if (!ctx) return CGP_E_ARG;
    return launch_on(ctx, prepare_gaussian_expectation(func, ms, sd, n, xi, w, order, out), kLaunchUnlocked, [&]() -> Verdict {
        const int64_t blocks = (n + 255) / 256;
        const unsigned grid = (unsigned)(blocks < 2048 ? blocks : 2048);
        hipStream_t st = (hipStream_t)stream;
        switch (func) {
        case CGP_FN_EXP:      hipLaunchKernelGGL(gaussian_expectation_kernel<CGP_FN_EXP>, dim3(grid), dim3(256), 0, st, ms, sd, n, in_stride, xi, w, order, out); break;
        case CGP_FN_IDENTITY: hipLaunchKernelGGL(gaussian_expectation_kernel<CGP_FN_IDENTITY>, dim3(grid), dim3(256), 0, st, ms, sd, n, in_stride, xi, w, order, out); break;
        case CGP_FN_SQUARE:   hipLaunchKernelGGL(gaussian_expectation_kernel<CGP_FN_SQUARE>, dim3(grid), dim3(256), 0, st, ms, sd, n, in_stride, xi, w, order, out); break;
        default:              hipLaunchKernelGGL(gaussian_expectation_kernel<CGP_FN_SOFTPLUS>, dim3(grid), dim3(256), 0, st, ms, sd, n, in_stride, xi, w, order, out); break;
        }
        return hip_rc(hipGetLastError());
    });
}

int cgp_squared_error_sums(cgp_ctx* ctx, const double* a, const double* r, int64_t B, int64_t T, int32_t d,
                           const int32_t* comps, int32_t n, double* sums, void* stream) {
    if (!ctx) return CGP_E_ARG;
    ErrComps ec{};
    return launch_on(ctx, prepare_squared_error_sums(a, r, B, T, d, comps, n, sums, ec), kLaunchUnlocked, [&]() -> Verdict {
        hipLaunchKernelGGL(squared_error_sums_kernel, dim3((unsigned)((T + 63) / 64), (unsigned)((B + 511) / 512)), dim3(256), 0, (hipStream_t)stream, a, r, B, T,
                           (int)d, ec, sums);
        return hip_rc(hipGetLastError());
    });
}

int cgp_pcrlb_sums(cgp_ctx* ctx, const cgp_model* model, double dt, const double* x0, const double* xs, int64_t B, int64_t T,
                   double* sums, uint32_t flags, void* stream) {
    if (!ctx) return CGP_E_ARG;
    PcrlbIO io{};
    ModelArgs ma;
    int key = 0;
    return launch_on(ctx, prepare_pcrlb_sums(model, dt, x0, xs, B, T, sums, flags, io, ma, key), kLaunchUnlocked, [&]() -> Verdict {
        const int rc = dispatch_pcrlb(model->model_id, key, io, ma, (hipStream_t)stream);
        if (rc == CGP_E_UNSUPPORTED) return {rc, "cgp_pcrlb_sums: this (model, dimension) combination is not compiled in"};
        return rc;
    });
}

int cgp_debug_math(cgp_ctx* ctx, int op, const double* x, int64_t n, double* out0, double* out1, void* stream) {
    if (!ctx) return CGP_E_ARG;
    return launch_on(ctx, prepare_debug_math(op, x, n, out0), kLaunchUnlocked, [&]() -> Verdict {
        const int64_t blocks = (n + 255) / 256;
        if (op == 5 || op == 6 || op == 8 || op == 16 || op == 17) hipLaunchKernelGGL(debug_math_uniform_kernel, dim3((unsigned)(n < 4096 ? n : 4096)), dim3(64), 0, (hipStream_t)stream, op, x, n, out0, out1);
        else hipLaunchKernelGGL(debug_math_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, op, x, n, out0, out1);
        return hip_rc(hipGetLastError());
    });
}

}  // extern "C"
