// cgp_args.hpp -- the pure half of every C-ABI entry point: prepare_<entry> takes the entry's arguments and what the context contributes
// (HostCtx) and answers with a Verdict -- a refusal (code and message), "nothing to do" (an empty batch or record), or "launch", with the
// launch description filled: the kernels' IO struct, their ModelArgs and, for cgp_filter / cgp_smoother, the decision of the route
// functions (cgp_route.hpp).  Host code without a HIP call or a device access, so a host program can ask it (tests/abi_probe.hip); the
// accepted path allocates nothing and builds no string (a refusal's message is a literal, or is written when refusing: refusef).
// The entry points (cgp_api.hip, cgp_rtc.hip, cgp_inst_sim.hip, cgp_inst_tangent4*.hip) are: null context, prepare_, launch_on
// (cgp_kernels.hpp) with what they enqueue.  Stated once, here: a model's expected shape (model_shape), the flags' names (flag_name) and
// the refusal that quotes one, the initial condition's four arrays (set_init), and every form of ModelArgs (model_args).
// Included by cgp_kernels.hpp, behind cgp_route.hpp.
#pragma once
#include "cgp_kernels.hpp"
#ifndef __HIPCC_RTC__          // host code (the run-time-compiled models include these headers)
#include <cstdarg>
#include <cstdio>

namespace cgp {

// What the context contributes to a launch description
struct HostCtx {
    int device = 0, num_cus = 256;
    int walk_segments = 0, lane_buffers = 0;         // cgp_debug_set
    unsigned long long* counters = nullptr;
};
inline HostCtx host_of(const cgp_ctx* ctx) { return {ctx->device, ctx->num_cus, ctx->walk_segments, ctx->lane_buffers, ctx->counters}; }

// A refusal whose message quotes an argument: written into the calling thread's buffer, which lives until its next such refusal
#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline Verdict refusef(int rc, const char* format, ...) {
    static thread_local char text[512];
    va_list args;
    va_start(args, format);
    vsnprintf(text, sizeof text, format, args);
    va_end(args);
    return {rc, text};
}
const Verdict kNothingToDo{CGP_OK, nullptr, true};

// ---- a model's expected shape, by model id ------------------------------------------------------------------------------------------
struct ModelShape {
    bool known, sde;
    int n_params, d;                 // what n_params and d have to be, given the model's d and n_harm
    int key;                         // what the dispatch tables go by: d for the linear models, n_harm for the harmonic / KPT ones
};
inline ModelShape model_shape(const cgp_model& m) {
    switch (m.model_id) {
    case CGP_M_LINEAR:       return {true, false, 2 * m.d * m.d, m.d, m.d};
    case CGP_M_KPT:          return {true, false, 2 * m.d * m.d, m.n_harm + 2, m.n_harm};
    case CGP_M_HARMONIC_LCD: return {true, false, 5, 2 * m.n_harm + 2, m.n_harm};
    case CGP_M_LASCALA_LCD:  return {true, false, 2, 4, 1};
    case CGP_M_LINEAR_SDE:   return {true, true, m.d * m.d, m.d, m.d};
    case CGP_M_HARMONIC_SDE: return {true, true, 3, 2 * m.n_harm + 2, m.n_harm};
    default:                 return {false, false, -1, m.d, m.d};
    }
}
inline Verdict check_model(const cgp_model* m, bool sde, bool need_sigma, const cgp_sigma* sg) {
    if (!m || !m->params) return {CGP_E_ARG, "model or model.params is NULL"};
    // dimensions above 8 are compiled in for the harmonic LCD model alone (4 and 5 harmonics: d = 10, 12)
    const int max_d = (m->model_id == CGP_M_HARMONIC_LCD) ? CGP_MAX_D : 8;
    if (m->d < 1 || m->d > max_d) return refusef(CGP_E_UNSUPPORTED, "state dimension outside 1..%d for this model", max_d);
    const ModelShape want = model_shape(*m);
    if (!want.known) return {CGP_E_ARG, "unknown model_id"};
    if (m->n_params != want.n_params) return {CGP_E_ARG, "model.n_params does not match model_id / d"};
    if (m->d != want.d) return {CGP_E_ARG, "model.d does not match model_id / n_harm"};
    if (m->param_stride != 0 && m->param_stride < m->n_params) return {CGP_E_ARG, "model.param_stride < n_params"};
    if (sde != want.sde) return {CGP_E_ARG, sde ? "continuous-discrete methods need an SDE model" : "discrete methods need a discrete (cond_m_cov) model"};
    if (sde && !m->gamma) return {CGP_E_ARG, "SDE methods need model.gamma = b b^T"};
    if (need_sigma) {
        if (!sg || !sg->xi || !sg->w || sg->s < 1) return {CGP_E_ARG, "sigma-point methods need a cgp_sigma"};
        if (sg->d != m->d) return {CGP_E_ARG, "cgp_sigma.d != model.d"};
        if (sg->group_start && (sg->n_groups < 1 || sg->n_groups > sg->s)) return {CGP_E_ARG, "cgp_sigma.n_groups outside 1..s"};
    }
    return {};
}

// ---- flags ----------------------------------------------------------------------------------------------------------------------------
// The header's name of one flag bit, for the message that refuses it
inline const char* flag_name(uint32_t bit) {
    if (bit & CGP_RK4_SUBSTEPS_MASK) return "CGP_RK4_SUBSTEPS";
    switch (bit) {
    case CGP_NLL_FINAL_ONLY: return "CGP_NLL_FINAL_ONLY";
    case CGP_WAVE_PER_TRIAL: return "CGP_WAVE_PER_TRIAL";
    case CGP_THREAD_PER_TRIAL: return "CGP_THREAD_PER_TRIAL";
    case CGP_SEQUENTIAL_SCAN: return "CGP_SEQUENTIAL_SCAN";
    case CGP_GENERIC_KERNEL: return "CGP_GENERIC_KERNEL";
    case CGP_SIM_FIXED_X0: return "CGP_SIM_FIXED_X0";
    case CGP_LITERAL_SIGMA_SUM: return "CGP_LITERAL_SIGMA_SUM";
    case CGP_DPP_KERNEL: return "CGP_DPP_KERNEL";
    case CGP_FOUR_TRIALS_PER_WAVE: return "CGP_FOUR_TRIALS_PER_WAVE";
    case CGP_ONE_TRIAL_PER_WAVE: return "CGP_ONE_TRIAL_PER_WAVE";
    case CGP_TIME_SPLIT: return "CGP_TIME_SPLIT";
    case CGP_NO_TIME_SPLIT: return "CGP_NO_TIME_SPLIT";
    case CGP_SKIP_MISSING: return "CGP_SKIP_MISSING";
    default: return "no flag of chirpgp_hip.h";
    }
}
// An entry point that takes no flag, or CGP_SKIP_MISSING alone (`taken`): the lowest bit it does not take, by value and by name
inline Verdict check_flags(const char* entry, uint32_t flags, uint32_t taken) {
    const uint32_t other = flags & ~taken;
    if (!other) return {};
    const uint32_t bit = other & (~other + 1u);
    return refusef(CGP_E_ARG, "%s takes %s: bit 0x%x (%s) is set", entry, taken ? "CGP_SKIP_MISSING and no other flag" : "no flag", (unsigned)bit,
                   flag_name(bit));
}

// ---- the pieces of a launch description -------------------------------------------------------------------------------------------------
// the initial condition and measurement model of FilterIO / TangentIO / SimIO
template <class IO> inline void set_init(IO& io, const cgp_init* init) {
    io.H = init->H; io.H_stride = init->H_stride;
    io.Xi = init->Xi; io.Xi_stride = init->Xi_stride;
    io.m0 = init->m0; io.m0_stride = init->m0_stride;
    io.P0 = init->P0; io.P0_stride = init->P0_stride;
}
template <class IO> inline void set_record(IO& io, const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index) {
    io.ys = ys; io.ys_stride = ys_stride; io.ys_repeat = ys_repeat; io.ys_index = ys_index;
}
// The kernels' view of a model and a sigma-point set (sg NULL: none).  `groups`: the set keeps its group table; `assertions`: and what the
// caller asserts of it (CGP_SIGMA_*).  Every ModelArgs is made here, through one of the four forms below, with every member set.  (The
// structs themselves carry no member initialisers: with them the kernels that copy a SigmaSet compiled to other code.)
inline ModelArgs model_args(const double* params, int64_t param_stride, const double* gamma, int64_t gamma_stride, int model_id, double dt,
                            const cgp_sigma* sg, bool groups, bool assertions) {
    ModelArgs a;
    a.params = params; a.param_stride = param_stride;
    a.gamma = gamma; a.gamma_stride = gamma_stride;
    a.model_id = model_id;
    a.sg.xi = nullptr; a.sg.w = nullptr; a.sg.group_start = nullptr; a.sg.s = 0; a.sg.n_groups = 0; a.sg.flags = 0u;
    a.sg.lds_xi = 0; a.sg.lds_w = 0; a.sg.lds_gs = 0; a.sg.lds_tab = 0;      // (set by SigmaSet::stage, in the kernel)
    if (sg) {
        a.sg.xi = sg->xi; a.sg.w = sg->w; a.sg.s = sg->s;
        if (groups && sg->group_start) { a.sg.group_start = sg->group_start; a.sg.n_groups = sg->n_groups; }
        if (assertions) a.sg.flags = sg->flags;
    }
    a.dt = dt;
    a.substeps = 1;
    return a;
}
// a filter's or smoother's (CGP_LITERAL_SIGMA_SUM: the set without its assertions; CGP_RK4_SUBSTEPS: n, and the kernels' dt is the substep
// h = dt / n -- one IEEE division, here; n = 1 leaves dt as it came)
inline ModelArgs model_args(const cgp_model* m, const cgp_sigma* sg, double dt, uint32_t flags) {
    ModelArgs a = model_args(m->params, m->param_stride, m->gamma, m->gamma_stride, m->model_id, dt, sg, true, !(flags & CGP_LITERAL_SIGMA_SUM));
    const int n = substeps_of(flags);
    if (n > 1) { a.substeps = n; a.dt = dt / (double)n; }
    return a;
}
// the literal per-point sums of kernels that take no groups (the tangent kernels, cgp_smoother_sample): a grouped set without its group table
inline ModelArgs model_args_literal(const cgp_model* m, const cgp_sigma* sg, double dt) {
    return model_args(m->params, m->param_stride, m->gamma, m->gamma_stride, m->model_id, dt, sg, false, false);
}
// a bare discrete model: no sigma-point set, no gamma (cgp_simulate, cgp_pcrlb_sums)
inline ModelArgs model_args_bare(const cgp_model* m, double dt) {
    return model_args(m->params, m->param_stride, nullptr, 0, m->model_id, dt, nullptr, false, false);
}
// a run-time-compiled model's: the set as a plain point list read from global memory -- no groups, no LDS stage, no closed forms
inline ModelArgs model_args_custom(const double* params, int64_t param_stride, const double* gamma, int64_t gamma_stride, double dt, const cgp_sigma* sg) {
    return model_args(params, param_stride, gamma, gamma_stride, -1, dt, sg, false, false);
}
// the selected outputs of a cgp_smooth_out as the kernels take them: in their SmootherIO, or as the argument of smooth_select_kernel
inline SmoothSel smooth_sel(const cgp_smooth_out& out) {
    SmoothSel sel;
    sel.comp = out.comp; sel.func = out.func; sel.order = out.order;
    sel.mean = out.comp_mean; sel.var = out.comp_var; sel.expect = out.expect; sel.xi = out.xi; sel.w = out.w;
    return sel;
}

// ---- cgp_filter, cgp_filter_time_split ----------------------------------------------------------------------------------------------------
struct FilterCall {
    int method;
    const cgp_model* model; const cgp_sigma* sigma; const cgp_init* init;
    double dt;
    const double* ys; int64_t ys_stride, ys_repeat; const int32_t* ys_index;
    int64_t B, T;
    double* mfs; double* Pfs; double* nll;
    uint32_t flags;
    bool time_split = false;                         // cgp_filter_time_split, with its three arguments
    int64_t segments = 1, burn_in = 0;
    double* junction_err = nullptr;
    const double* dts = nullptr; int64_t dts_stride = 0;      // cgp_filter_timed (include/chirpgp_hip_timed.h): one interval per step; dt is not read
    bool timed = false;
};
struct FilterPlan {
    FilterIO io{};                                   // complete but for the workspace of the segment records (seg_state)
    ModelArgs ma;
    FilterDecision route;
};
inline Verdict prepare_filter(const FilterCall& c, const HostCtx& h, FilterPlan& p) {
    if (c.time_split) {
        if (c.segments < 1) return {CGP_E_ARG, "segments must be >= 1"};
        if (c.flags & CGP_SKIP_MISSING)
            return {CGP_E_UNSUPPORTED, "CGP_SKIP_MISSING goes with cgp_filter and cgp_filter_custom only: a time-split filter's burn-in that starts "
                                       "inside a gap has no junction to compare"};
        if (c.flags & CGP_RK4_SUBSTEPS_MASK) return {CGP_E_UNSUPPORTED, kSubstepsSplit};
        if (c.timed) return {CGP_E_UNSUPPORTED, kTimedSplit};
    }
    if (c.B < 0 || c.T < 0) return {CGP_E_ARG, "negative B or T"};
    if (c.B == 0 || c.T == 0) return kNothingToDo;
    if (!c.ys) return {CGP_E_ARG, "ys is NULL"};
    if (c.ys_stride < 0) return {CGP_E_ARG, "ys_stride must be >= 0 (T for dense [B][T] records, 0 for one shared record)"};
    if (c.ys_repeat < 1) return {CGP_E_ARG, "ys_repeat must be >= 1"};
    if (c.timed) {
        if (!c.dts) return {CGP_E_ARG, "dts is NULL"};
        if (c.dts_stride < 0) return {CGP_E_ARG, "dts_stride must be >= 0 (T for one time grid per record, 0 for one shared grid)"};
    }
    if (!c.init || !c.init->Xi || !c.init->m0 || !c.init->P0) return {CGP_E_ARG, "init.Xi / m0 / P0 must be set"};
    if (c.method != CGP_F_EKF_KPT && !c.init->H) return {CGP_E_ARG, "init.H must be set"};
    const bool sde = c.method == CGP_F_CD_EKF || c.method == CGP_F_CD_SGP;
    const bool sig = c.method == CGP_F_SGP || c.method == CGP_F_CD_SGP;
    if (c.method < CGP_F_EKF || c.method > CGP_F_EKF_KPT) return {CGP_E_ARG, "unknown filter method"};
    if (c.timed && (!sde || (c.model && !model_shape(*c.model).sde))) return {CGP_E_ARG, kTimedDiscrete};
    if (const Verdict v = check_model(c.model, sde, sig, c.sigma); v.rc != CGP_OK) return v;
    if ((c.method == CGP_F_EKF_KPT) != (c.model->model_id == CGP_M_KPT)) return {CGP_E_ARG, "CGP_F_EKF_KPT goes with CGP_M_KPT only"};
    const bool split = c.segments > 1;
    if (split) {
        if (c.burn_in < 0) return {CGP_E_ARG, "burn_in must be >= 0"};
        if (!c.junction_err) return {CGP_E_ARG, "junction_err must be set: a time-split filter is only as good as its junctions"};
    }
    FilterIO& io = p.io;
    set_init(io, c.init);
    set_record(io, c.ys, c.ys_stride, c.ys_repeat, c.ys_index);
    io.B = c.B; io.T = c.T; io.mfs = c.mfs; io.Pfs = c.Pfs; io.nll = c.nll; io.flags = c.flags;
    io.counters = h.counters;
    if (c.timed) { io.dts = c.dts; io.dts_stride = c.dts_stride; }
    p.ma = model_args(c.model, c.sigma, c.dt, c.flags);
    p.route = route_filter({c.method, c.model, c.sigma, &io, &p.ma, c.flags, c.segments, h.num_cus, c.timed});
    if (p.route.rc != CGP_OK) return {p.route.rc, p.route.message};
    io.flags = p.route.flags;
    if (split) {
        // time-split with burn-in (cgp_filter_time_split): segments of whole 64-step chunks, one wavefront each
        io.segs = p.route.segs; io.seg_len = p.route.seg_len; io.burn_in = (c.burn_in + 63) / 64 * 64;
        io.seg_stride = seg_layout(c.model->d).stride;
    }
    return {};
}

// ---- cgp_smoother, cgp_smoother_select, cgp_smoother_time_split ----------------------------------------------------------------------------
struct SmootherCall {
    int method;
    const cgp_model* model; const cgp_sigma* sigma;
    double dt;
    const double* mfs; const double* Pfs;
    int64_t B, T;
    const cgp_smooth_out* out;
    uint32_t flags;
    bool time_split = false;                         // cgp_smoother_time_split, with its three arguments
    int64_t segments = 1, burn_in = 0;
    double* junction_err = nullptr;
    // cgp_smoother_timed (include/chirpgp_hip_timed.h): one interval per step, with an addressing of their own; dt is not read
    const double* dts = nullptr; int64_t dts_stride = 0, dts_repeat = 1; const int32_t* dts_index = nullptr;
    bool timed = false;
};
struct SmootherPlan {
    SmootherIO io{};                                 // complete but for the workspace of the junction states (junction)
    ModelArgs ma;
    SmootherDecision route;
    SmoothSel sel;                                   // the selected outputs, for the gather launch too
};
inline Verdict prepare_smoother(const SmootherCall& c, const HostCtx& h, SmootherPlan& p) {
    if (c.time_split) {
        if (c.segments < 1) return {CGP_E_ARG, "segments must be >= 1"};
        if (!c.junction_err) return {CGP_E_ARG, "junction_err must be set"};
        if (c.flags & CGP_RK4_SUBSTEPS_MASK) return {CGP_E_UNSUPPORTED, kSubstepsSplit};
        if (c.timed) return {CGP_E_UNSUPPORTED, kTimedSplit};
    }
    if (c.B < 0 || c.T < 0) return {CGP_E_ARG, "negative B or T"};
    if (c.B == 0 || c.T == 0) return kNothingToDo;
    if (!c.out) return {CGP_E_ARG, "out is NULL"};
    const cgp_smooth_out& out = *c.out;
    const bool want_sel = out.comp_mean || out.comp_var || out.expect;
    if (c.timed) {
        if (!c.dts) return {CGP_E_ARG, "dts is NULL"};
        if (c.dts_stride < 0) return {CGP_E_ARG, "dts_stride must be >= 0 (T for one time grid per trial, 0 for one shared grid)"};
        if (c.dts_repeat < 1) return {CGP_E_ARG, "dts_repeat must be >= 1"};
    }
    if (!c.mfs || !c.Pfs) return {CGP_E_ARG, "mfs / Pfs must be set"};
    if (!want_sel && (!out.mss || !out.Pss)) return {CGP_E_ARG, "mfs / Pfs / mss / Pss must be set"};
    if (want_sel) {
        if (!c.model || out.comp < 0 || out.comp >= c.model->d) return {CGP_E_ARG, "cgp_smooth_out.comp outside 0..d-1"};
        if (out.expect && (out.func < CGP_FN_SOFTPLUS || out.func > CGP_FN_SQUARE || out.order < 1 || out.order > kGhMaxOrder || !out.xi || !out.w))
            return {CGP_E_ARG, "cgp_smooth_out.expect needs func, 1 <= order <= 32, xi and w"};
    }
    if (c.method < CGP_S_EKS || c.method > CGP_S_CD_SGP) return {CGP_E_ARG, "unknown smoother method"};
    const bool sde = c.method == CGP_S_CD_EKS || c.method == CGP_S_CD_SGP;
    const bool sig = c.method == CGP_S_SGP || c.method == CGP_S_CD_SGP;
    if (c.timed && (!sde || (c.model && !model_shape(*c.model).sde))) return {CGP_E_ARG, kTimedDiscrete};
    if (const Verdict v = check_model(c.model, sde, sig, c.sigma); v.rc != CGP_OK) return v;
    if (c.model->model_id == CGP_M_KPT) return {CGP_E_ARG, "the KPT model has no smoother in the reference"};
    SmootherIO& io = p.io;
    io.mfs = c.mfs; io.Pfs = c.Pfs; io.B = c.B; io.T = c.T; io.mss = out.mss; io.Pss = out.Pss; io.flags = c.flags;
    p.ma = model_args(c.model, c.sigma, c.dt, c.flags);
    // the whole plan -- kernel, launch shape, segments, how the selected outputs get written -- decided before anything is enqueued
    SmootherQuery query{c.method, c.model, c.sigma, &io, &p.ma, c.flags, h.num_cus};
    query.walk_cap = h.walk_segments;
    query.segments = c.segments; query.burn_in = c.burn_in;
    query.want_sel = want_sel; query.null_rows = !out.mss || !out.Pss;
    query.timed = c.timed;
    if (c.timed) { io.dts = c.dts; io.dts_stride = c.dts_stride; io.dts_repeat = c.dts_repeat; io.dts_index = c.dts_index; }
    p.route = route_smoother(query);
    if (p.route.rc != CGP_OK) return {p.route.rc, p.route.message};
    p.sel = smooth_sel(out);
    if (p.route.select == SmootherSelect::kKernel) io.sel = p.sel;
    if (p.route.bsegs > 1) {
        // time-split with burn-in (cgp_smoother_time_split): one wavefront per (trial, segment), their states at the junctions for the fix-up pass
        io.bsegs = p.route.bsegs; io.chunks_per_bseg = p.route.chunks_per_bseg; io.burn_chunks = p.route.burn_chunks;
    }
    return {};
}

// ---- cgp_smoother_sample ------------------------------------------------------------------------------------------------------------------------
inline Verdict prepare_smoother_sample(int method, const cgp_model* model, const cgp_sigma* sigma, double dt, const double* mfs, const double* Pfs,
                                       int64_t B, int64_t T, int64_t S, uint64_t seed, int64_t trial0, int64_t sample0, const double* normals,
                                       const cgp_sample_out* out, uint32_t flags, SampleIO& io, ModelArgs& ma) {
    if (B < 0 || T < 0 || S < 0) return {CGP_E_ARG, "negative B, T or S"};
    if (const Verdict v = check_flags("cgp_smoother_sample", flags, 0); v.rc != CGP_OK) return v;
    if (B == 0 || T == 0 || S == 0) return kNothingToDo;                   // nothing to write
    if (!out || (!out->paths && !out->comp_paths)) return {CGP_E_ARG, "cgp_sample_out.paths and comp_paths are both NULL: nothing to write"};
    if (method < CGP_S_EKS || method > CGP_S_CD_SGP) return {CGP_E_ARG, "unknown smoother method"};
    if (method == CGP_S_CD_EKS || method == CGP_S_CD_SGP)
        return {CGP_E_UNSUPPORTED, "cgp_smoother_sample walks the discrete smoothers' affine maps (rts, eks, sgp_smoother): a continuous-discrete "
                                   "smoother's backward ODE is not such a map"};
    const bool sig = method == CGP_S_SGP;
    if (const Verdict v = check_model(model, false, sig, sigma); v.rc != CGP_OK) return v;
    const bool lcd = (model->model_id == CGP_M_HARMONIC_LCD && model->n_harm == 1) || model->model_id == CGP_M_LASCALA_LCD;
    const bool built = model->d == 4 && (lcd || (model->model_id == CGP_M_LINEAR && method == CGP_S_EKS));
    if (!built)
        return {CGP_E_UNSUPPORTED, "cgp_smoother_sample is built for d = 4: rts on CGP_M_LINEAR, eks and sgp_smoother on CGP_M_HARMONIC_LCD with n_harm = 1 "
                                   "and CGP_M_LASCALA_LCD"};
    if (sig && SigmaSet::stage_bytes(sigma->s, 4, 0, false) > (size_t)kSigLdsMaxBytes)
        return {CGP_E_UNSUPPORTED, "the sigma-point set does not fit the LDS stage of cgp_smoother_sample"};
    if (out->comp_paths) {
        if (out->comp < 0 || out->comp >= model->d) return {CGP_E_ARG, "cgp_sample_out.comp outside 0..d-1"};
        if (out->func < CGP_FN_SOFTPLUS || out->func > CGP_FN_SQUARE) return {CGP_E_ARG, "cgp_sample_out.func is no CGP_FN_*"};
    }
    const uint64_t two32 = (uint64_t)1 << 32;
    if (B > 0x7FFFFFFF) return {CGP_E_ARG, "B must be < 2^31 (one workgroup column per trial)"};
    if (!normals) {                                                        // the counter's words: (trial, sample, index)
        if (trial0 < 0 || sample0 < 0) return {CGP_E_ARG, "negative trial0 or sample0"};
        if ((uint64_t)trial0 + (uint64_t)B > two32) return {CGP_E_ARG, "trial0 + B must be <= 2^32 (the trial is one word of the Philox counter)"};
        if ((uint64_t)sample0 + (uint64_t)S > two32) return {CGP_E_ARG, "sample0 + S must be <= 2^32 (the sample is one word of the Philox counter)"};
        if ((uint64_t)T > two32 / 2) return {CGP_E_ARG, "T * ceil(d / 2) must be <= 2^32 (the pair index is one word of the Philox counter)"};
    }
    if (!mfs || !Pfs) return {CGP_E_ARG, "mfs / Pfs must be set"};
    io.mfs = mfs; io.Pfs = Pfs; io.normals = normals; io.B = B; io.T = T; io.S = S;
    io.seed = seed; io.trial0 = (uint64_t)trial0; io.sample0 = (uint64_t)sample0;
    io.paths = out->paths; io.comp_paths = out->comp_paths; io.comp = out->comp_paths ? out->comp : 0; io.func = out->func;
    ma = model_args_literal(model, sig ? sigma : nullptr, dt);
    return {};
}

// ---- the tangent entry points: cgp_ekf_nll_grad / _fisher, cgp_sgp_nll_grad / _fisher, cgp_cd_ekf_nll_grad ------------------------------------
struct TangentCall {
    const char* entry;                   // the entry point's name, for its messages
    bool sgp, fisher;                    // takes a sigma-point set (sigma-point sets beyond the LDS stage are refused; with an SDE model: the
                                         // continuous-discrete sigma-point form, cgp_tangent4_cd_sigma.hpp) / writes the matrix
    bool cd = false;                     // the continuous-discrete form (cgp_tangent4_cd.hpp): the d = 4 chirp / La Scala SDE with its gamma
};
// The argument checks in the ABI's order (flags last: CGP_SKIP_MISSING or nothing), then what the entry's own grid can hold.  Nothing to do:
// B == 0 or n_dir == 0, decided before anything else is looked at (T == 0 launches: nll = 0, grad = 0).
inline Verdict prepare_tangent(TangentCall call, const cgp_model* model, const cgp_sigma* sigma, const cgp_init* init, double dt,
                               const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index, int64_t B, int64_t T,
                               const double* dirs, int32_t n_dir, double* nll, double* grad, double* fisher, uint32_t flags, TangentIO& io, ModelArgs& ma) {
    const char* entry = call.entry;
    if (B < 0 || T < 0 || n_dir < 0) return {CGP_E_ARG, "negative B, T or n_dir"};
    if (B == 0 || n_dir == 0) return kNothingToDo;
    if (call.fisher && n_dir > CGP_FISHER_MAX_DIR)      // a row of the matrix lives in registers, and the matrix couples all the directions of a launch
        return refusef(CGP_E_UNSUPPORTED, "%s takes all directions in one launch: n_dir must be <= CGP_FISHER_MAX_DIR (16)", entry);
    if (!model || !model->params) return {CGP_E_ARG, "model or model.params is NULL"};
    const ModelShape want = model_shape(*model);
    const bool shaped = model->n_harm == 1 && model->n_params == want.n_params && model->d == want.d;      // (n_harm = 1: d = 4)
    // the sigma-point entry points take their continuous-discrete form from the MODEL: an SDE model is cd_sgp_filter's (cgp_tangent4_cd_sigma.hpp)
    const bool cd_sgp = call.sgp && model->model_id == CGP_M_HARMONIC_SDE;
    if (call.cd) {
        if (model->model_id != CGP_M_HARMONIC_SDE || !shaped || !model->gamma)
            return refusef(CGP_E_UNSUPPORTED, "%s is built for the d = 4 chirp and La Scala SDE (CGP_M_HARMONIC_SDE, n_harm = 1) with model.gamma set", entry);
        if (model->gamma_stride != 0 && model->gamma_stride < 16) return {CGP_E_ARG, "model.gamma_stride < d * d"};
    } else if (cd_sgp) {
        if (call.fisher)
            return refusef(CGP_E_UNSUPPORTED, "%s: the Fisher form of the continuous-discrete filters is not built (CGP_M_HARMONIC_SDE goes with cgp_sgp_nll_grad)", entry);
        if (!shaped || !model->gamma)
            return refusef(CGP_E_UNSUPPORTED, "%s takes CGP_M_HARMONIC_SDE with n_harm = 1, d = 4, n_params = 3 and model.gamma set: the d = 4 chirp and La Scala SDE", entry);
        if (model->gamma_stride != 0 && model->gamma_stride < 16) return {CGP_E_ARG, "model.gamma_stride < d * d"};
    } else {
        const bool chirp = model->model_id == CGP_M_HARMONIC_LCD && shaped;
        const bool lascala = model->model_id == CGP_M_LASCALA_LCD && model->n_params == want.n_params && model->d == want.d;
        if (!chirp && !lascala) return refusef(CGP_E_UNSUPPORTED, "%s is built for the d = 4 chirp and La Scala LCD models", entry);
    }
    if (model->param_stride != 0 && model->param_stride < model->n_params) return {CGP_E_ARG, "model.param_stride < n_params"};
    if (call.sgp) {
        if (!sigma) return {CGP_E_ARG, "sigma is NULL"};
        if (sigma->d != 4) return refusef(CGP_E_UNSUPPORTED, "%s is built for d = 4 sigma-point sets", entry);
        if (!sigma->xi || !sigma->w || sigma->s < 1) return {CGP_E_ARG, "cgp_sigma.xi / w must be set and s >= 1"};
        // (the continuous-discrete form parks its RK4 step's state in LDS beside the set)
        if (SigmaSet::stage_bytes(sigma->s, 4, 0, false) + (cd_sgp ? (size_t)kCdSgpParkBytes : 0) > (size_t)kSigLdsMaxBytes)
            return refusef(CGP_E_UNSUPPORTED, "the sigma-point set does not fit the LDS stage of %s", entry);
    }
    if (!init || !init->H || !init->Xi || !init->m0 || !init->P0) return {CGP_E_ARG, "init.H / Xi / m0 / P0 must be set"};
    if (T > 0 && !ys) return {CGP_E_ARG, "ys is NULL"};
    if (ys_stride < 0 || ys_repeat < 1) return {CGP_E_ARG, "ys_stride must be >= 0 and ys_repeat >= 1"};
    if (!dirs || !nll || !grad || (call.fisher && !fisher))
        return {CGP_E_ARG, call.fisher ? "dirs / nll / grad / fisher must be set" : "dirs / nll / grad must be set"};
    // the one flag these entry points take; the continuous-discrete forms take CGP_RK4_SUBSTEPS beside it
    const bool rk4 = call.cd || cd_sgp;
    if (const Verdict v = check_flags(entry, rk4 ? flags & ~CGP_RK4_SUBSTEPS_MASK : flags, CGP_SKIP_MISSING); v.rc != CGP_OK) return v;
    // the grids: one workgroup per trial (sigma-point), 64 / n_dir whole trials per wavefront (the EKF's Fisher form), B n_dir lanes (cd)
    if (call.sgp) {
        if (B > 0x7fffffffLL) return refusef(CGP_E_UNSUPPORTED, "%s runs one workgroup per trial: B must be < 2^31", entry);
    } else if (call.fisher) {
        if ((B + (64 / n_dir) - 1) / (64 / n_dir) > 0x7fffffffLL) return refusef(CGP_E_UNSUPPORTED, "%s: too many trials for one grid", entry);
    } else if (call.cd) {
        if (B > (0x7fffffffLL * 64) / n_dir) return refusef(CGP_E_UNSUPPORTED, "%s: too many lanes (B n_dir) for one grid", entry);
    }
    set_init(io, init);
    set_record(io, ys, ys_stride, ys_repeat, ys_index);
    io.dirs = dirs; io.B = B; io.T = T; io.n_dir = n_dir; io.nll = nll; io.grad = grad; io.fisher = call.fisher ? fisher : nullptr;
    ma = model_args_literal(model, call.sgp ? sigma : nullptr, dt);
    if (const int n = substeps_of(flags); rk4 && n > 1) { ma.substeps = n; ma.dt = dt / (double)n; }          // (as model_args(..., flags))
    return {};
}

// ---- cgp_filter_custom, cgp_smoother_custom: what they need to know of a cgp_custom_model (cgp_rtc.hip), as plain values ------------------------
struct CustomModel {
    bool present = false;                // the caller's pointer is not NULL
    int kind = 0, d = 0, device = 0;
    bool ekf = false, sgp = false;       // the entry's kernel exists in the model's code object: without / with a sigma-point set
};
// CGP_RK4_SUBSTEPS on a run-time compiled model: an SDE model's (CGP_CUSTOM_SDE) alone -- n, and h = dt / n as the kernels' dt, as
// model_args(..., flags) has them
inline Verdict custom_substeps(const CustomModel& m, uint32_t flags, double dt, ModelArgs& ma) {
    const int n = substeps_of(flags);
    if (n == 1) return {};
    if (m.kind != CGP_CUSTOM_SDE) return {CGP_E_ARG, kSubstepsDiscrete};
    ma.substeps = n; ma.dt = dt / (double)n;
    return {};
}
inline Verdict check_custom_sigma(const cgp_sigma* sigma, int d) {
    if (sigma && (!sigma->xi || !sigma->w || sigma->s < 1 || sigma->d != d)) return {CGP_E_ARG, "cgp_sigma needs xi, w, s >= 1 and d = the model's"};
    return {};
}
inline Verdict prepare_filter_custom(const CustomModel& m, const cgp_sigma* sigma, const double* params, int64_t param_stride, const double* gamma,
                                     int64_t gamma_stride, const cgp_init* init, double dt, const double* ys, int64_t ys_stride, int64_t ys_repeat,
                                     const int32_t* ys_index, int64_t B, int64_t T, double* mfs, double* Pfs, double* nll, uint32_t flags,
                                     const HostCtx& h, FilterIO& io, ModelArgs& ma) {
    if (!m.present) return {CGP_E_ARG, "model is NULL"};
    if (B < 0 || T < 0) return {CGP_E_ARG, "negative B or T"};
    if (B == 0 || T == 0) return kNothingToDo;
    if (m.device != h.device) return {CGP_E_ARG, "the model was compiled for another device's context"};
    if (!ys || !params) return {CGP_E_ARG, "ys / params is NULL"};
    if (ys_stride < 0 || ys_repeat < 1) return {CGP_E_ARG, "ys_stride must be >= 0 and ys_repeat >= 1"};
    if (!init || !init->H || !init->Xi || !init->m0 || !init->P0) return {CGP_E_ARG, "init.H / Xi / m0 / P0 must be set"};
    if (m.kind == CGP_CUSTOM_SDE && !gamma) return {CGP_E_ARG, "SDE models need gamma = b b^T"};
    if (!(sigma ? m.sgp : m.ekf)) return {CGP_E_UNSUPPORTED, "a measurement function (ekf_for_kpt) has no sigma-point form"};
    if (const Verdict v = check_custom_sigma(sigma, m.d); v.rc != CGP_OK) return v;
    if ((flags & CGP_RK4_SUBSTEPS_MASK) && m.kind != CGP_CUSTOM_SDE) return {CGP_E_ARG, kSubstepsDiscrete};
    set_init(io, init);
    set_record(io, ys, ys_stride, ys_repeat, ys_index);
    io.B = B; io.T = T; io.mfs = mfs; io.Pfs = Pfs; io.nll = nll; io.flags = flags & (CGP_NLL_FINAL_ONLY | CGP_SKIP_MISSING);
    ma = model_args_custom(params, param_stride, gamma, gamma_stride, dt, sigma);
    return custom_substeps(m, flags, dt, ma);
}
inline Verdict prepare_smoother_custom(const CustomModel& m, const cgp_sigma* sigma, const double* params, int64_t param_stride, const double* gamma,
                                       int64_t gamma_stride, double dt, const double* mfs, const double* Pfs, int64_t B, int64_t T, double* mss,
                                       double* Pss, uint32_t flags, const HostCtx& h, SmootherIO& io, ModelArgs& ma) {
    if (!m.present) return {CGP_E_ARG, "model is NULL"};
    if (B < 0 || T < 0) return {CGP_E_ARG, "negative B or T"};
    if (B == 0 || T == 0) return kNothingToDo;
    if (m.device != h.device) return {CGP_E_ARG, "the model was compiled for another device's context"};
    if (!mfs || !Pfs || !mss || !Pss || !params) return {CGP_E_ARG, "mfs / Pfs / mss / Pss / params must be set"};
    if (m.kind == CGP_CUSTOM_SDE && !gamma) return {CGP_E_ARG, "SDE models need gamma = b b^T"};
    if (!(sigma ? m.sgp : m.ekf))
        return {CGP_E_UNSUPPORTED, "a measurement function (ekf_for_kpt) has no smoother of its own: its dynamics are linear -- cgp_smoother with CGP_S_EKS on (F, Sigma)"};
    if (const Verdict v = check_custom_sigma(sigma, m.d); v.rc != CGP_OK) return v;
    if (flags & CGP_RK4_SUBSTEPS_MASK) {
        if (m.kind != CGP_CUSTOM_SDE) return {CGP_E_ARG, kSubstepsDiscrete};
        // (one wavefront per trial, the set staged in LDS beside the table of the interval's moments: route_smoother's condition)
        if (sigma && SigmaSet::stage_bytes(sigma->s, m.d, 0, false) + substep_table_bytes(m.d) > (size_t)kSigLdsMaxBytes)
            return {CGP_E_UNSUPPORTED, "CGP_RK4_SUBSTEPS: the sigma-point set does not fit the LDS stage beside the table of intermediate moments"};
    }
    io.mfs = mfs; io.Pfs = Pfs; io.B = B; io.T = T; io.mss = mss; io.Pss = Pss; io.flags = flags;
    ma = model_args_custom(params, param_stride, gamma, gamma_stride, dt, sigma);
    return custom_substeps(m, flags, dt, ma);
}

// ---- cgp_simulate, cgp_simulate_x0, cgp_add_noise ------------------------------------------------------------------------------------------------
struct SimShape { int key = 0; bool wave = true; };      // the dispatch key, and one wavefront or one lane per trial
inline Verdict prepare_simulate(const cgp_model* model, const cgp_init* init, double dt, uint64_t seed, int64_t trial0, int64_t B, int64_t T,
                                double* xs, double* ys, uint32_t flags, const HostCtx& h, SimIO& io, ModelArgs& ma, SimShape& shape) {
    if (B < 0 || T < 0 || trial0 < 0) return {CGP_E_ARG, "negative B, T or trial0"};
    if (B == 0 || T == 0) return kNothingToDo;
    if (!xs && !ys) return {CGP_E_ARG, "xs and ys are both NULL"};
    if (!model || !model->params) return {CGP_E_ARG, "model or model.params is NULL"};
    if (!init || !init->m0 || (!init->P0 && !(flags & CGP_SIM_FIXED_X0))) return {CGP_E_ARG, "init.m0 / P0 must be set"};
    if (ys && (!init->H || !init->Xi)) return {CGP_E_ARG, "measurements need init.H and init.Xi"};
    const ModelShape want = model_shape(*model);
    if (!want.known || want.sde || model->model_id == CGP_M_KPT) return {CGP_E_ARG, "cgp_simulate takes a discrete (cond_m_cov) model"};
    if (model->d < 1 || model->d > CGP_MAX_D || model->d != want.d) return {CGP_E_ARG, "model.d does not match model_id / n_harm"};
    if (model->n_params != want.n_params) return {CGP_E_ARG, "model.n_params does not match model_id / d"};
    if (model->param_stride != 0 && model->param_stride < model->n_params) return {CGP_E_ARG, "model.param_stride < n_params"};
    // counter word 2 holds step * ceil(d / 2) + pair
    if ((uint64_t)T * (uint64_t)((model->d + 1) / 2) > 0xFFFFFFFFull) return {CGP_E_ARG, "T too long for the 32-bit step counter"};
    set_init(io, init);
    io.seed = seed; io.trial0 = trial0; io.B = B; io.T = T; io.xs = xs; io.ys = ys;
    io.vec_ok = 0; io.flags = flags;
    if (xs && ((uintptr_t)xs & 15) == 0 && ((T * model->d) & 1) == 0) io.vec_ok |= 1;
    if (ys && ((uintptr_t)ys & 15) == 0 && (T & 1) == 0) io.vec_ok |= 2;
    ma = model_args_bare(model, dt);
    shape.key = want.key;
    // One wavefront per trial draws the noise of 64 steps in parallel and pays ~160 replicated instructions per step;
    // one lane per trial pays the ~750 instructions of a step once per 64 trials: crossover near 8 waves per SIMD.
    shape.wave = B < (int64_t)h.num_cus * 4 * 8;
    if (flags & CGP_WAVE_PER_TRIAL) shape.wave = true;
    if (flags & CGP_THREAD_PER_TRIAL) shape.wave = false;
    return {};
}
inline Verdict prepare_simulate_x0(const cgp_model* model, const cgp_init* init, int64_t trial0, int64_t B, const double* x0) {
    if (B < 0 || trial0 < 0) return {CGP_E_ARG, "negative B or trial0"};
    if (B == 0) return kNothingToDo;
    if (!model) return {CGP_E_ARG, "model is NULL (its d is the state dimension)"};
    if (!init || !init->m0 || !init->P0) return {CGP_E_ARG, "init.m0 / P0 must be set"};
    if (!x0) return {CGP_E_ARG, "x0 is NULL"};
    if (model->d < 1 || model->d > 8) return {CGP_E_UNSUPPORTED, "cgp_simulate_x0: state dimension outside 1..8"};
    return {};
}
inline Verdict prepare_add_noise(const double* clean, int64_t clean_stride, const double* Xi, int64_t trial0, int64_t B, int64_t T, const double* ys) {
    if (B < 0 || T < 0 || trial0 < 0) return {CGP_E_ARG, "negative B, T or trial0"};
    if (B == 0 || T == 0) return kNothingToDo;
    if (!clean || !Xi || !ys) return {CGP_E_ARG, "NULL pointer"};
    if (clean_stride != 0 && clean_stride < T) return {CGP_E_ARG, "clean_stride < T"};
    if ((uint64_t)T > 0x1FFFFFFFEull) return {CGP_E_ARG, "T too long for the 32-bit step counter"};
    return {};
}

// ---- cgp_gaussian_expectation_fn, cgp_squared_error_sums -------------------------------------------------------------------------------------
inline Verdict prepare_gaussian_expectation(int func, const double* ms, const double* sd, int64_t n, const double* xi, const double* w, int32_t order,
                                            const double* out) {
    if (func < CGP_FN_SOFTPLUS || func > CGP_FN_SQUARE) return {CGP_E_ARG, "unknown integrand"};
    if (n < 0 || order < 1) return {CGP_E_ARG, "bad n or order"};
    if (n == 0) return kNothingToDo;
    if (!ms || !sd || !xi || !w || !out) return {CGP_E_ARG, "NULL pointer"};
    return {};
}
struct ErrComps { int c[8]; int n; };                // the components squared_error_sums_kernel sums (comps is the HOST's array)
inline Verdict prepare_squared_error_sums(const double* a, const double* r, int64_t B, int64_t T, int32_t d, const int32_t* comps, int32_t n,
                                          const double* sums, ErrComps& ec) {
    if (B < 0 || T < 0 || d < 1 || n < 1 || n > 8) return {CGP_E_ARG, "bad B, T, d or n (1 <= n <= 8)"};
    if (B == 0 || T == 0) return kNothingToDo;
    if (!a || !r || !comps || !sums) return {CGP_E_ARG, "NULL pointer"};
    ec.n = n;
    for (int i = 0; i < 8; i++) {
        ec.c[i] = i < n ? comps[i] : 0;
        if (ec.c[i] < 0 || ec.c[i] >= d) return {CGP_E_ARG, "component outside 0..d-1"};
    }
    if ((B + 511) / 512 > 65535) return {CGP_E_ARG, "more than 65535 x 512 trials in one call: reduce chunk by chunk"};
    return {};
}

// ---- cgp_pcrlb_sums ---------------------------------------------------------------------------------------------------------------------------------
inline Verdict prepare_pcrlb_sums(const cgp_model* model, double dt, const double* x0, const double* xs, int64_t B, int64_t T, double* sums,
                                  uint32_t flags, PcrlbIO& io, ModelArgs& ma, int& key) {
    if (B < 0 || T < 0) return {CGP_E_ARG, "negative B or T"};
    if (const Verdict v = check_flags("cgp_pcrlb_sums", flags, 0); v.rc != CGP_OK) return v;
    if (B == 0 || T == 0) return kNothingToDo;                             // nothing to add
    if (!model || !model->params) return {CGP_E_ARG, "model or model.params is NULL"};
    if (!x0 || !xs || !sums) return {CGP_E_ARG, "NULL pointer: x0, xs and sums are all needed"};
    if (model->model_id == CGP_M_LASCALA_LCD)
        return {CGP_E_UNSUPPORTED, "cgp_pcrlb_sums: the transition of CGP_M_LASCALA_LCD has a singular Sigma and so no density to differentiate"};
    if (model->model_id != CGP_M_LINEAR && model->model_id != CGP_M_HARMONIC_LCD)
        return {CGP_E_UNSUPPORTED, "cgp_pcrlb_sums takes CGP_M_LINEAR and CGP_M_HARMONIC_LCD: a Gaussian transition with a constant Sigma and a linear measurement"};
    if (const Verdict v = check_model(model, false, false, nullptr); v.rc != CGP_OK) return v;
    if (model->param_stride != 0) return {CGP_E_ARG, "cgp_pcrlb_sums: model.param_stride must be 0 (the expectation is over the samples of ONE model)"};
    if (model->d > 8) return {CGP_E_UNSUPPORTED, "cgp_pcrlb_sums is compiled for d <= 8 (CGP_M_HARMONIC_LCD: n_harm <= 3)"};
    if ((B + kPcrlbSlab - 1) / kPcrlbSlab > 65535) return {CGP_E_ARG, "more than 65535 x 512 trials in one call: accumulate chunk by chunk"};
    io.x0 = x0; io.xs = xs; io.B = B; io.T = T; io.sums = sums;
    ma = model_args_bare(model, dt);
    key = model_shape(*model).key;
    return {};
}

// ---- cgp_debug_math, cgp_debug_philox -----------------------------------------------------------------------------------------------------------
inline bool debug_math_pairs(int op) { return op == 22 || op == 23 || op == 25; }      // two-argument ops: (x[2 i], x[2 i + 1]) -> o0[i], o1[i]
inline Verdict prepare_debug_math(int op, const double* x, int64_t n, const double* out0) {
    if (n < 0 || op < 0 || op > 25) return {CGP_E_ARG, "bad op or n"};
    if (debug_math_pairs(op) && (n & 1)) return {CGP_E_ARG, "a two-argument op takes an even number of inputs"};
    if (n == 0) return kNothingToDo;
    if (!x || !out0) return {CGP_E_ARG, "NULL pointer"};
    return {};
}
inline Verdict prepare_debug_philox(const uint32_t* ctr, const uint32_t* key, int64_t n, const uint32_t* out) {
    if (n < 0) return {CGP_E_ARG, "negative n"};
    if (n == 0) return kNothingToDo;
    if (!ctr || !key || !out) return {CGP_E_ARG, "NULL pointer"};
    return {};
}

}  // namespace cgp
#endif                         // __HIPCC_RTC__
