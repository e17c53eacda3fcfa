// cgp_route.hpp -- which kernel a cgp_filter / cgp_smoother call runs, and its whole launch plan: the refusals that depend on the kernel,
// the segments of the time-split forms (with burn-in: both entries; exact: walk_split_policy and walk_segments for the cooperative walks,
// whose launcher only adds the occupancy it has to ask the runtime for) and how a smoother's selected outputs get written.  Host code
// without a HIP call or a device access: the C-ABI (cgp_api.hip) asks route_filter / route_smoother before it enqueues anything, and a
// host program can ask them too (tests/route_probe.hip).  Each kernel's admission predicate is stated once, here, and serves the route
// functions and the guard of the kernel's launcher alike.  Included by cgp_kernels.hpp, behind the types it needs.
#pragma once
#include "cgp_kernels.hpp"
#ifndef __HIPCC_RTC__          // host code (the run-time-compiled models include these headers)

namespace cgp {

// ---- admission: what each specialised kernel can address -------------------------------------------------------------------------
// Outputs leave through raw-buffer windows (cgp_coop4.hpp: OobWindow) of at most 2 GiB less the last line: whatever one workgroup
// addresses through one window -- `bytes_per_step` for each of T steps -- has to fit.
constexpr int64_t kOobMaxBytes = 0x7FFFFF00;
inline bool oob_fits(int64_t T, int64_t bytes_per_step) { return T * bytes_per_step <= kOobMaxBytes; }

// d = 4 on the matrix cores (cgp_mfma4*.hpp): one trial's covariance rows a window, four trials' in the four-trials-per-wavefront EKF
inline bool mfma4_rows_fit(int64_t T) { return oob_fits(T, 128); }
inline bool ekf4_mfma_fits(const FilterIO& io) { return mfma4_rows_fit(io.T); }
inline bool ekf4_mfma_x4_fits(const FilterIO& io) { return oob_fits(io.T, 512); }
// The collapsed quadrature of the d = 4 sigma-point kernels needs the caller's CGP_SIGMA_STANDARD assertion, groups, and one group per
// lane of a half wave; the matrix-core kernels (cgp_mfma4_sigma.hpp, cgp_mfma4_cd.hpp) are built for it alone.
inline bool collapsed_ok(const ModelArgs& ma) {
    return (ma.sg.flags & CGP_SIGMA_STANDARD) && ma.sg.group_start && ma.sg.n_groups >= 1 && ma.sg.n_groups <= 32;
}
inline bool sgp4_mfma_fits(int64_t T, const ModelArgs& ma) { return collapsed_ok(ma) && mfma4_rows_fit(T); }

// d = 6 / 8 in the 8 x 8 tile layout (cgp_coop8.hpp) and ekf_for_kpt (cgp_kpt8.hpp): one trial's d x d rows a window.  The
// sigma-point filter's collapsed quadrature: the standard-set assertion, groups, at most one group per (DPP row, block) pair.
inline bool coop8_rows_fit(int d, int64_t T) { return oob_fits(T, (int64_t)d * d * 8); }
inline bool coop8_sigma_ok(const ModelArgs& ma) {
    return (ma.sg.flags & CGP_SIGMA_STANDARD) && ma.sg.group_start && ma.sg.n_groups >= 1 && ma.sg.n_groups <= 16;
}
inline bool coop8_filter_sgp_ok(int n_harm, int64_t T, const ModelArgs& ma) {
    return (n_harm == 2 || n_harm == 3) && coop8_sigma_ok(ma) && coop8_rows_fit(2 * n_harm + 2, T);
}
inline bool kpt8_fits(int n_harm, int64_t T) { return coop8_rows_fit(n_harm + 2, T); }
// The cooperative smoother keeps 16 step records and the tile's 64 filtering rows in 36.9 KB of static LDS (the split kernel:
// 32 records, 27.9 KB); with the staged sigma-point set beside it a workgroup must stay within 40 KB so that four of them
// (one per SIMD) share a CU's 160 KB (every cubature rule fits; larger sets take the lane-scan kernel).
constexpr size_t kCoop8SmootherLdsBytes = sizeof(double) * (16 * 109 + 64 * 45);      // cgp_coop8.hpp: 16 kElemDoubles + 64 kRowDoubles
inline bool coop8_smoother_ok(int d, int64_t T, const ModelArgs& ma) {
    return d >= 5 && d <= 8 && coop8_rows_fit(d, T) && sigma_lds_bytes(ma, d) + kCoop8SmootherLdsBytes + 64 <= 40 * 1024;
}
// the sigma-point elements of the harmonic models are compiled in their collapsed form only: other sets take the lane-scan kernel
inline bool coop8_smoother_harm_ok(int method, const ModelArgs& ma) {
    return method == CGP_S_EKS || (method == CGP_S_SGP && (ma.sg.flags & CGP_SIGMA_STANDARD) && ma.sg.group_start);
}
// The d = 4 walk (cgp_walk4.hpp): one workgroup holds 64 records (18 944 B) beside the staged sigma-point set; at least four of them
// have to share a CU's 160 KB.
constexpr size_t kWalk4LdsBytes = sizeof(double) * 64 * 37;                             // cgp_walk4.hpp: 64 kWalkRec
inline bool walk4_smoother_ok(int64_t T, const ModelArgs& ma) {
    return mfma4_rows_fit(T) && sigma_lds_bytes(ma, 4) + kWalk4LdsBytes + 64 <= 40 * 1024;
}

// d = 4, one lane per trial, large batches (cgp_lane4.hpp).  The launches it takes: dense or shared records whose rows start on
// 16-byte boundaries (its LDS-DMA moves 16-byte pieces), an even number of steps, output windows of 64 trials within the 2 GiB a
// raw buffer addresses, no time-split segments ...
inline bool lane4_filter_fits(const FilterIO& io) {
    return io.segs <= 1 && io.T >= 2 && io.T % 2 == 0 && io.ys_stride % 2 == 0 && ((uintptr_t)io.ys & 15) == 0 && oob_fits(io.T, 128 * 64);
}
// ... for its sigma-point filter a set that fits beside the kernel's static LDS (cgp_steps.hpp) ...
inline bool lane4_sgp_fits(const ModelArgs& ma) { return sigma_lds_bytes(ma, 4) <= (size_t)kLane4SigLdsMaxBytes; }
// ... and its smoothers (eks on the chirp / La Scala LCD models, cd_eks on the chirp SDE): 16-byte aligned inputs (LDS-DMA), output
// windows of 64 trials within 2 GiB
inline bool lane4_smoother_fits(const SmootherIO& io) {
    return io.T >= 2 && oob_fits(io.T, 128 * 64) && ((uintptr_t)io.mfs & 15) == 0 && ((uintptr_t)io.Pfs & 15) == 0;
}

// ---- launch shape ------------------------------------------------------------------------------------------------------------------
// One wavefront per trial is the latency-optimal shape while the batch is about the number of
// SIMDs (1024): a step then costs its dependent-instruction chain once.  One lane per trial costs more per step but
// carries 64 trials per wave, so it wins as soon as enough wavefronts would have to share a SIMD -- how many depends on how
// much faster the lane-cooperative (matrix-core) kernel's step is than the one-lane step.  Crossovers measured on MI355X in
// round 3 (bench.py --batch B --flags 2 | 4; wave-per-trial time grows linearly with B beyond 1024, the lane-per-trial time is
// flat until B ~ 64 K), in trials per SIMD:
//     EKF, chirp / La Scala d = 4 (MFMA, four trials per wave above 1024)   1.25 ms vs 2.58 at 8 K, 2.29 vs 2.65 at 16 K, 3.33 vs 2.89 at 24 K   -> 20
//     EKF, 2 / 3 harmonics d = 6 / 8 (tile layout)                          0.93 vs 1.81 at 4 K, 1.73 vs 1.82 at 8 K, 3.29 vs 1.88 at 16 K        -> 8
//     sigma-point filter, d = 4 (MFMA sums)                                 1.38 vs 8.17 at 4 K, 5.12 vs 8.18 at 16 K, 6.2 vs 5.1 at 32 K         -> 24
//     sigma-point filter, d = 6 / 8 (tile layout)                           2.52 vs 6.95 at 4 K, 9.58 vs 6.99 at 16 K                             -> 11
//     cd_ekf / cd_eks, d = 4 (MFMA)                                         1.41 vs 1.38 / 1.38 vs 1.90 at 4 K, 4.95 vs 1.40 / 4.89 vs 2.07 at 16 K -> 4 / 5
//     cd_sgp filter / smoother, d = 4 (MFMA)                                2.3 vs 28.6 at 4 K, 9.2 vs 28.7 at 16 K                               -> 48
//     discrete smoothers on the cooperative walks (d = 4 .. 8)              never slower than one lane per trial: 0.36 vs 9.98 ms (sigma-point d = 4,
//                                                                           4 K), 2.77 vs 18.4 (EKS d = 8, 16 K), 9.4 vs 10.6 (EKS d = 4, 256 K)   -> always
//     everything on the generic kernels                                     as measured in round 1: 2.5 (EKF-type), 8 (sigma-point), 16 (affine scan)
// Round 5, where the large-batch lane kernel of cgp_lane4.hpp is what one lane per trial runs: it wins from 9 / 9 trials per SIMD on
// (tools/lane_crossover.sh, profiles/r05_lane_crossover.txt: EKF 0.49 against 0.59 ms at 8192 x 500 and 0.71 against 0.59 at 10 240 --
// CRLB records, i.e. with the four-trials-per-wavefront kernel on its branch-free wide step --, GH-3 4.3 against 5.0 ms at 8192 x 500
// and 6.5 against 5.0 at 12 288, after the lane kernel's fan stopped running twice on records outside the lean regime; the generic
// lane kernel it replaces there kept the round-3 limits of 20 / 24).  Smoothers: eks on the d = 4 chirp models beyond 24 trials per
// SIMD -- 1.21 against 1.48 ms at 32 768 x 500, 8.0 against 10.6 ms at 262 144 x 500, the walk ahead below: 0.70 against 0.93 ms at
// 16 384; profiles/r05_lane_smoothers.txt -- and cd_eks from 3: 1.74 against 2.48 ms at 4096 x 500.
// Calls with CGP_SKIP_MISSING (tools/gaps_probe.py, flagged launches at T = 500 on 1024 SIMDs, one wavefront against one lane per trial,
// the lane shape being the generic kernel's -- the large-batch lane kernels know no gaps):
//     EKF, chirp d = 4 (the kernel for gaps, one trial per wave)             0.40 ms vs 0.92 at 2 K, 0.73 vs 0.99 at 4 K, 1.37 vs 1.01 at 8 K, 2.60 vs 1.04 at 16 K
//                                                                           (linear in between: equal near 5.7 K trials)                         -> 11 / 2
//     sigma-point filter GH-3, d = 4 (MFMA sums, GAPS form)                  0.73 vs 6.94 at 2 K, 1.41 vs 7.02 at 4 K, 2.74 vs 7.01 at 8 K, 5.32 vs 7.01 at 16 K
//                                                                           (0.314 us a trial beyond: equal near 21.8 K, not measured there;
//                                                                           other sets go by GH-3's figure, as they do unflagged)               -> 21
// Every other flagged call -- cd_ekf, cd_sgp_filter, whatever the generic kernel runs -- is unmeasured and goes by the generic limits
// ({5, 2}, sigma-point {8, 1}) whatever kernel it takes (route_filter).
struct ShapeLimit { int num, den; };                      // one wavefront per trial while B * den < num * SIMDs; num < 0: always
constexpr ShapeLimit kWaveAlways{-1, 1};
inline bool choose_wave(int num_cus, int64_t B, uint32_t flags, ShapeLimit limit, const cgp_sigma* sg) {
    // the wave-per-trial shapes stage the sigma-point set in LDS; a set that does not fit runs one lane per trial
    if (sg && SigmaSet::stage_bytes(sg->s, sg->d, sg->n_groups, sg->group_start != nullptr) > (size_t)kSigLdsMaxBytes) return false;
    if (flags & CGP_WAVE_PER_TRIAL) return true;
    if (flags & CGP_THREAD_PER_TRIAL) return false;
    if (limit.num < 0) return true;
    const int64_t simds = (int64_t)num_cus * 4;
    return B * limit.den < (int64_t)limit.num * simds;
}
// What a call would run with one wavefront per trial, and up to how many trials per SIMD that beats what it would run with one lane
// per trial: `limit` against a generic lane kernel, `limit_lane4` against the large-batch kernels of cgp_lane4.hpp.
template <class Route> struct WaveCandidate {
    Route route;
    ShapeLimit limit, limit_lane4;
    void crossover(int trials_per_simd, int against_lane4) { limit = {trials_per_simd, 1}; limit_lane4 = {against_lane4, 1}; }
};

// ---- filters -----------------------------------------------------------------------------------------------------------------------
enum class FilterRoute {
    kGenericWave, kGenericLane,                                // filter_kernel of cgp_kernels.hpp, by model family and method
    kKf4Mfma,                                                  // kf at d = 4: the matrix-core EKF step with the constant Jacobian F
    kEkf4Mfma, kEkf4MfmaSeg, kEkf4MfmaX4, kEkf4Coop,           // ekf, d = 4: one trial, one segment or four trials a wavefront; DPP rows
    kSgp4Mfma, kSgp4Coop, kLane4Ekf, kLane4Sgp,                // sgp_filter, d = 4; the large-batch lane kernels
    kEkf8Coop, kSgp8Coop,                                      // 2 / 3 harmonics in the tile layout
    kCdEkf4Mfma, kCdEkf4Coop, kCdSgp4Mfma, kCdSgp4Coop,        // continuous-discrete, d = 4
    kKpt8Coop, kGenericKpt                                     // ekf_for_kpt: tile layout / matrix cores, or filter_kernel in either shape
};
// CGP_SKIP_MISSING (include/chirpgp_hip.h, cgp_filter): a flagged call may only reach a kernel that honours the flag -- filter_kernel in
// both shapes (the gate of scalar_update, cgp_math.hpp) and the one-wavefront-per-trial matrix-core kernels at d = 4, whose launchers
// take the EKF's kernel for records with gaps or the GAPS instantiation of the others (cgp_inst_gaps4.hip, cgp_inst_gaps4_sigma.hip).
// Every other route is replaced by the generic kernel of the shape the call has (route_filter).
inline bool honours_gaps(FilterRoute r) {
    return r == FilterRoute::kGenericWave || r == FilterRoute::kGenericLane || r == FilterRoute::kGenericKpt || r == FilterRoute::kEkf4Mfma ||
           r == FilterRoute::kSgp4Mfma || r == FilterRoute::kCdEkf4Mfma || r == FilterRoute::kCdSgp4Mfma;
}
// CGP_RK4_SUBSTEPS (include/chirpgp_hip.h): likewise -- filter_kernel in both shapes on SubstepPredict (cgp_steps.hpp), which the generic
// routes launch for a flagged call (cgp_inst_substeps_*.hip), and the one-wavefront-per-trial matrix-core kernels of cd_ekf and cd_sgp_filter
// at d = 4, whose launchers take the SUB instantiation, with GAPS or without (cgp_inst_substeps4.hip).  The DPP kernels take one RK4 step
// per sample: a flagged call is handed to the generic kernel of the shape it has.  The crossovers of flagged calls are unmeasured and go
// by the generic limits whatever kernel they take, as those of CGP_SKIP_MISSING on these two methods do.
inline int substeps_of(uint32_t flags) { return (int)((flags & CGP_RK4_SUBSTEPS_MASK) >> 16) + 1; }
inline bool honours_substeps(FilterRoute r) {
    return r == FilterRoute::kGenericWave || r == FilterRoute::kGenericLane || r == FilterRoute::kCdEkf4Mfma || r == FilterRoute::kCdSgp4Mfma;
}
constexpr const char* kSubstepsDiscrete = "CGP_RK4_SUBSTEPS goes with the continuous-discrete methods only (cd_ekf, cd_sgp_filter, cd_eks, cd_sgp_smoother): "
                                          "a discrete model has no ODE to integrate";
constexpr const char* kSubstepsSplit = "CGP_RK4_SUBSTEPS goes with cgp_filter, cgp_smoother and cgp_smoother_select only: the time-split kernels take one RK4 "
                                       "step per sample";
// Timed calls (include/chirpgp_hip_timed.h: one interval per step): likewise -- filter_kernel in both shapes on TimedPredict
// (cgp_steps.hpp; cgp_inst_timed_*.hip) and the one-wavefront-per-trial matrix-core kernels of cd_ekf and cd_sgp_filter at d = 4, whose
// launchers take the TIMED instantiation, with GAPS and SUB or without (cgp_inst_timed4.hip).  A timed call is routed like the untimed
// call with the same flags -- kernel, launch shape, crossover -- and where that ends on any other kernel (the DPP forms, a large-batch lane
// kernel) it takes the generic kernel in the shape the call has.
inline bool honours_times(FilterRoute r) {
    return r == FilterRoute::kGenericWave || r == FilterRoute::kGenericLane || r == FilterRoute::kCdEkf4Mfma || r == FilterRoute::kCdSgp4Mfma;
}
constexpr const char* kTimedDiscrete = "per-step intervals go with the continuous-discrete methods on an SDE model only (cd_ekf, cd_sgp_filter, cd_eks, "
                                       "cd_sgp_smoother): a discrete model's constants are fixed per dt at set-up";
constexpr const char* kTimedSplit = "there is no timed form of the time-split entry points: their kernels take one dt";
// the kernels that know the segments of a time-split launch (kEkf4Mfma: as kEkf4MfmaSeg)
inline bool knows_segments(FilterRoute r) {
    return r == FilterRoute::kEkf4Mfma || r == FilterRoute::kSgp4Mfma || r == FilterRoute::kSgp8Coop || r == FilterRoute::kCdSgp4Mfma;
}
struct FilterQuery {
    int method;
    const cgp_model* model;          // checked (check_model)
    const cgp_sigma* sigma;          // or NULL
    const FilterIO* io;              // filled but for the segments
    const ModelArgs* ma;
    uint32_t flags;
    int64_t segments;                // requested (cgp_filter_time_split); 1: none
    int num_cus;
    bool timed = false;              // cgp_filter_timed: one interval per step (FilterIO::dts)
};
struct FilterDecision {
    int rc = CGP_OK;                 // or the refusal and its message
    const char* message = nullptr;
    FilterRoute route = FilterRoute::kGenericWave;
    bool wave = true;
    uint32_t flags = 0;              // the call's, with CGP_WAVE_PER_TRIAL where the segments force it
    int segs = 1;                    // effective: without the empty ones
    bool gaps = false;               // CGP_SKIP_MISSING: the launcher of a matrix-core route takes the kernel's GAPS instantiation
    int64_t seg_len = 0;
    bool substeps = false;           // CGP_RK4_SUBSTEPS: the generic routes launch their SubstepPredict instantiation
    bool timed = false;              // cgp_filter_timed: the generic and the cd matrix-core routes launch their TIMED instantiation
};

inline WaveCandidate<FilterRoute> filter_wave_candidate(const FilterQuery& q) {
    const cgp_model& m = *q.model;
    const int64_t T = q.io->T;
    const bool sig = q.method == CGP_F_SGP || q.method == CGP_F_CD_SGP;
    const ShapeLimit generic = sig ? ShapeLimit{8, 1} : ShapeLimit{5, 2};
    WaveCandidate<FilterRoute> c{FilterRoute::kGenericWave, generic, generic};
    const bool spec = !(q.flags & CGP_GENERIC_KERNEL), mfma = !(q.flags & CGP_DPP_KERNEL);
    // Kept as found: a crossover belongs to the (method, model) family and the flags, not to the kernel the family ends up with -- a record
    // too long for a matrix-core or tile-layout kernel's windows, or a set its quadrature does not take, runs the DPP or generic kernel
    // under the specialised kernel's limit (d = 6 / 8: {8, 1} and {11, 1} on the generic kernel), CGP_DPP_KERNEL and
    // CGP_ONE_TRIAL_PER_WAVE fall back to the generic limits, and kf at d = 4 never left them.
    switch (m.model_id) {
    case CGP_M_LINEAR:
        if (q.method == CGP_F_EKF && m.d == 4 && spec && mfma && mfma4_rows_fit(T)) c.route = FilterRoute::kKf4Mfma;
        break;
    case CGP_M_HARMONIC_LCD:
    case CGP_M_LASCALA_LCD: {
        const bool chirp4 = spec && m.n_harm == 1;
        const bool harm8 = spec && m.model_id == CGP_M_HARMONIC_LCD && (m.n_harm == 2 || m.n_harm == 3);
        if (q.method == CGP_F_EKF && chirp4) {
            c.route = (mfma && ekf4_mfma_fits(*q.io)) ? FilterRoute::kEkf4Mfma : FilterRoute::kEkf4Coop;
            if (mfma && !(q.flags & CGP_ONE_TRIAL_PER_WAVE)) c.crossover(20, 9);
        } else if (q.method == CGP_F_SGP && chirp4) {
            c.route = (mfma && sgp4_mfma_fits(T, *q.ma)) ? FilterRoute::kSgp4Mfma : FilterRoute::kSgp4Coop;
            if (mfma) c.crossover(24, 9);
        } else if (q.method == CGP_F_EKF && harm8) {
            if (coop8_rows_fit(m.d, T)) c.route = FilterRoute::kEkf8Coop;
            c.crossover(8, 8);
        } else if (q.method == CGP_F_SGP && harm8) {
            if (coop8_filter_sgp_ok(m.n_harm, T, *q.ma)) c.route = FilterRoute::kSgp8Coop;
            c.crossover(11, 11);
        }
        break;
    }
    case CGP_M_HARMONIC_SDE: {
        const bool sde4 = spec && m.n_harm == 1;
        if (q.method == CGP_F_CD_SGP && sde4) {
            c.route = (mfma && sgp4_mfma_fits(T, *q.ma)) ? FilterRoute::kCdSgp4Mfma : FilterRoute::kCdSgp4Coop;
            if (mfma) c.crossover(48, 48);
        } else if (q.method == CGP_F_CD_EKF && sde4) {
            c.route = (mfma && mfma4_rows_fit(T)) ? FilterRoute::kCdEkf4Mfma : FilterRoute::kCdEkf4Coop;
            if (mfma) c.crossover(4, 4);
        }
        break;
    }
    case CGP_M_KPT:
        c.route = (spec && kpt8_fits(m.n_harm, T)) ? FilterRoute::kKpt8Coop : FilterRoute::kGenericKpt;
        break;
    default: break;
    }
    return c;
}
inline FilterRoute filter_lane_candidate(const FilterQuery& q, int segs) {
    const cgp_model& m = *q.model;
    if (m.model_id == CGP_M_KPT) return FilterRoute::kGenericKpt;
    const bool lcd = m.model_id == CGP_M_HARMONIC_LCD || m.model_id == CGP_M_LASCALA_LCD;
    if (lcd && m.n_harm == 1 && !(q.flags & CGP_GENERIC_KERNEL) && segs <= 1 && lane4_filter_fits(*q.io)) {
        if (q.method == CGP_F_EKF) return FilterRoute::kLane4Ekf;
        if (q.method == CGP_F_SGP && lane4_sgp_fits(*q.ma)) return FilterRoute::kLane4Sgp;
    }
    return FilterRoute::kGenericLane;
}
inline FilterDecision route_filter(const FilterQuery& q) {
    FilterDecision d;
    d.flags = q.flags;
    auto refuse = [&d](const char* message) { d.rc = CGP_E_UNSUPPORTED; d.message = message; return d; };
    const bool sig = q.method == CGP_F_SGP || q.method == CGP_F_CD_SGP;
    const int64_t B = q.io->B, T = q.io->T;
    WaveCandidate<FilterRoute> wave = filter_wave_candidate(q);
    d.gaps = (q.flags & CGP_SKIP_MISSING) != 0;
    if (d.gaps) {
        if (q.segments > 1)
            return refuse("CGP_SKIP_MISSING goes with cgp_filter and cgp_filter_custom only: a time-split filter's burn-in that starts inside a gap "
                          "has no junction to compare");
        if (!honours_gaps(wave.route)) wave.route = q.model->model_id == CGP_M_KPT ? FilterRoute::kGenericKpt : FilterRoute::kGenericWave;
        // the crossovers of flagged calls (see the measured ones above): against the generic lane kernel in every case
        wave.limit = wave.route == FilterRoute::kEkf4Mfma ? ShapeLimit{11, 2} : wave.route == FilterRoute::kSgp4Mfma ? ShapeLimit{21, 1}
                     : sig ? ShapeLimit{8, 1} : ShapeLimit{5, 2};
        wave.limit_lane4 = wave.limit;
    }
    d.substeps = (q.flags & CGP_RK4_SUBSTEPS_MASK) != 0;
    if (d.substeps) {
        if (q.method != CGP_F_CD_EKF && q.method != CGP_F_CD_SGP) { d.rc = CGP_E_ARG; d.message = kSubstepsDiscrete; return d; }
        if (q.segments > 1) return refuse(kSubstepsSplit);
        if (!honours_substeps(wave.route)) wave.route = FilterRoute::kGenericWave;
        wave.limit = wave.limit_lane4 = sig ? ShapeLimit{8, 1} : ShapeLimit{5, 2};      // unmeasured: the generic limits
    }
    // ---- time-split with burn-in (cgp_filter_time_split): segments of whole 64-step chunks, one wavefront each
    if (q.segments > 1) {
        // (kept as found: admission goes by the REQUESTED segments -- a record too short to split is refused all the same where the
        // kernel knows no segments -- and CGP_DPP_KERNEL refuses the split on the 2- / 3-harmonic model too, whose kernel has no DPP
        // variant to ask for)
        if (!knows_segments(wave.route) || (q.flags & (CGP_DPP_KERNEL | CGP_THREAD_PER_TRIAL | CGP_FOUR_TRIALS_PER_WAVE)))
            return refuse("time-split filters are built for ekf / sgp_filter / cd_sgp_filter on the d = 4 chirp and La Scala models "
                          "and sgp_filter on the 2- / 3-harmonic model (matrix-core and tile-layout kernels, standard sigma sets)");
        d.seg_len = ((T + q.segments - 1) / q.segments + 63) / 64 * 64;
        const int64_t segs = (T + d.seg_len - 1) / d.seg_len;              // without the empty ones
        if (segs > 1) {
            // (a set too large for the LDS stage runs one lane per trial whatever the flags say -- choose_wave -- and those kernels
            // know no segments: refuse instead of reading records nobody wrote)
            if (sig && SigmaSet::stage_bytes(q.sigma->s, q.sigma->d, q.sigma->n_groups, q.sigma->group_start != nullptr) > (size_t)kSigLdsMaxBytes)
                return refuse("time-split filters need a sigma-point set that fits the LDS stage of the one-wavefront-per-trial kernels");
            d.segs = (int)segs;
            d.flags |= CGP_WAVE_PER_TRIAL;
        }
    }
    FilterRoute lane = filter_lane_candidate(q, d.segs);
    if (d.gaps && !honours_gaps(lane)) lane = FilterRoute::kGenericLane;
    if (d.substeps && !honours_substeps(lane)) lane = FilterRoute::kGenericLane;
    const bool lane4 = lane == FilterRoute::kLane4Ekf || lane == FilterRoute::kLane4Sgp;
    d.wave = choose_wave(q.num_cus, B, d.flags, lane4 ? wave.limit_lane4 : wave.limit, sig ? q.sigma : nullptr);
    // (kept as found: unreachable -- the segments set CGP_WAVE_PER_TRIAL, and the one thing that overrides it was refused above)
    if (d.segs > 1 && !d.wave) return refuse("time-split filters run one wavefront per trial only");
    d.route = d.wave ? wave.route : lane;
    d.timed = q.timed;
    if (d.timed) {
        const int id = q.model->model_id;
        if ((q.method != CGP_F_CD_EKF && q.method != CGP_F_CD_SGP) || (id != CGP_M_LINEAR_SDE && id != CGP_M_HARMONIC_SDE)) {
            d.rc = CGP_E_ARG; d.message = kTimedDiscrete; return d;
        }
        if (q.segments > 1) return refuse(kTimedSplit);
        if (!honours_times(d.route)) d.route = d.wave ? FilterRoute::kGenericWave : FilterRoute::kGenericLane;
    }
    if (d.route == FilterRoute::kEkf4Mfma) {
        // beyond one wave per SIMD the four MFMA blocks carry four trials (CGP_ONE_TRIAL_PER_WAVE keeps one, for tests).  Kept as found:
        // "one wave per SIMD" is the literal 1024, whatever num_cus says.
        if (d.segs > 1) d.route = FilterRoute::kEkf4MfmaSeg;
        else if (d.gaps) d.route = FilterRoute::kEkf4Mfma;        // (the four-trials-per-wavefront kernel knows no gaps)
        else if ((B > 1024 || (q.flags & CGP_FOUR_TRIALS_PER_WAVE)) && ekf4_mfma_x4_fits(*q.io) && !(q.flags & CGP_ONE_TRIAL_PER_WAVE))
            d.route = FilterRoute::kEkf4MfmaX4;
    }
    return d;
}

// ---- smoothers ---------------------------------------------------------------------------------------------------------------------
enum class SmootherRoute {
    kCoop8Linear, kWalk4Linear, kDiscLinear,                   // rts: tile layout (5 <= d <= 8), the d = 4 walk, the generic kernels
    kCoop8Harm, kWalk4Harm, kLane4, kDiscHarm,                 // eks / sgp_smoother on the chirp family; kLane4 also cd_eks on the chirp SDE
    kSdeLinear, kCdSgp4Mfma, kCdSgp4Coop, kCdEks4Mfma, kCdEks4Coop, kSdeHarm, kNone
};
// selected outputs (cgp_smoother_select) are written by the kernel itself where it is one of the d = 4 walks / lane kernels or the
// tile-layout kernels (mss / Pss then optional); any other kernel writes the full rows and a gather launch reads the marginal back
inline bool writes_selection(SmootherRoute r) {
    return r == SmootherRoute::kWalk4Linear || r == SmootherRoute::kWalk4Harm || r == SmootherRoute::kLane4 || r == SmootherRoute::kCoop8Linear ||
           r == SmootherRoute::kCoop8Harm;
}
// the kernels that know the segments of a time-split launch with burn-in (cgp_smoother_time_split)
inline bool knows_segments(SmootherRoute r) { return r == SmootherRoute::kCdSgp4Mfma || r == SmootherRoute::kCdEks4Mfma; }
// the cooperative walks, whose launcher (launch_walk_smoother, cgp_coop8.hpp) knows the exact time split of the discrete smoothers
inline bool splits_exactly(SmootherRoute r) {
    return r == SmootherRoute::kWalk4Linear || r == SmootherRoute::kWalk4Harm || r == SmootherRoute::kCoop8Linear || r == SmootherRoute::kCoop8Harm;
}
struct SmootherQuery {
    int method;
    const cgp_model* model;          // checked (check_model)
    const cgp_sigma* sigma;          // or NULL
    const SmootherIO* io;            // mfs, Pfs, B, T
    const ModelArgs* ma;
    uint32_t flags;
    int num_cus;
    int walk_cap = 0;                // the context's CGP_DBG_WALK_SEGMENTS: 0 = choose, 1 = no exact split, n = at most n segments
    int64_t segments = 1;            // requested (cgp_smoother_time_split); 1: none
    int64_t burn_in = 0;
    bool want_sel = false;           // cgp_smoother_select: selected outputs are wanted ...
    bool null_rows = false;          // ... and mss or Pss is NULL
    bool timed = false;              // cgp_smoother_timed: one interval per step (SmootherIO::dts)
};
enum class SmootherSelect { kNone, kKernel, kGather };      // selected outputs: none, written by the kernel, gathered from the full rows (smooth_select_kernel)
struct SmootherDecision {
    int rc = CGP_OK;                 // or the refusal and its message
    const char* message = nullptr;
    SmootherRoute route = SmootherRoute::kNone;
    bool wave = true;
    SmootherSelect select = SmootherSelect::kNone;
    WalkSplit split;                 // the exact time split of the cooperative walks (walk_segments); off on every other route
    int bsegs = 1, chunks_per_bseg = 0, burn_chunks = 0;      // time split with burn-in, as SmootherIO has them; bsegs <= 1: nothing is split
    bool substeps = false;           // CGP_RK4_SUBSTEPS: kSdeLinear / kSdeHarm launch their SubstepSmooth instantiation
    bool timed = false;              // cgp_smoother_timed: kSdeLinear / kSdeHarm / kCdEks4Mfma / kCdSgp4Mfma launch their TIMED instantiation
};
// Timed calls (include/chirpgp_hip_timed.h): smoother_kernel in both shapes on TimedSmooth (cgp_steps.hpp) -- around SubstepSmooth with
// CGP_RK4_SUBSTEPS, one wavefront per trial as untimed -- and the matrix-core walks of cd_eks and cd_sgp_smoother at d = 4
// (cgp_inst_timed4_smoothers.hip).  A timed call whose untimed twin ends on another kernel (the DPP forms, the large-batch lane kernel)
// takes the generic kernel in the shape the call has.
inline bool honours_times(SmootherRoute r) {
    return r == SmootherRoute::kSdeLinear || r == SmootherRoute::kSdeHarm || r == SmootherRoute::kCdEks4Mfma || r == SmootherRoute::kCdSgp4Mfma;
}
// CGP_RK4_SUBSTEPS on a smoother: smoother_kernel on SubstepSmooth (cgp_steps.hpp), one wavefront per trial whatever the batch -- the
// interval's moments are a table in LDS, (d + d (d + 1) / 2) 16 doubles a wavefront (5.6 KB at d = 8), and 64 trials' tables do not fit.
// The matrix-core, DPP and lane smoothers take one RK4 step per sample: a flagged call is handed to the generic kernel in that shape.
inline bool honours_substeps(SmootherRoute r, bool wave) { return wave && (r == SmootherRoute::kSdeLinear || r == SmootherRoute::kSdeHarm); }
// (the table is static LDS of the kernel, sized for n = 16 whatever the call's n: so is this admission figure)
inline size_t substep_table_bytes(int d) { return sizeof(double) * (size_t)(d + d * (d + 1) / 2) * kMaxSubsteps; }      // cgp_steps.hpp: SubTable

// ---- the exact time split of the discrete wave-per-trial smoothers
// Whether a launch splits: when the batch leaves two thirds of the SIMDs idle, or on request (CGP_TIME_SPLIT, which also lets a
// segment be a single tile).  `walk_cap` caps the number of segments of a context (tuning aid).
inline WalkSplit walk_split_policy(const cgp_model& model, uint32_t flags, int64_t B, int num_cus, int walk_cap) {
    const bool forced = (flags & CGP_TIME_SPLIT) != 0;
    // Not by default for the LINEAR model (rts): its F is the caller's, and composing the affine maps of hundreds of steps
    // (C = Pf - G Pp G^T, A <- G A) is only as accurate as those products are well conditioned -- 1e-11 of the whole-record
    // walk for the chirp family's gains (d = 4 ... 8, every parameter set of the tests), but 1e-7 for a random F at d = 6,
    // where partial products of the gains grow in directions the true carry never excites.  The split is exact in exact
    // arithmetic either way; for a linear model it is the caller's choice (CGP_TIME_SPLIT).
    const bool own_model = model.model_id != CGP_M_LINEAR;
    WalkSplit s;
    if ((flags & CGP_NO_TIME_SPLIT) || (!forced && (!own_model || 3 * B > (int64_t)num_cus * 4))) s.cap = 1;      // measured: x3 at B = 125, x1.6 at 250, x0.9 at 500
    else s.cap = walk_cap > 1 ? walk_cap : (walk_cap == 1 ? 1 : 0);
    s.min_tiles = forced ? 1 : 4;
    return s;
}
// Wavefronts per trial and 64-step tiles per wavefront: as many as keep every workgroup resident at once (`blocks_per_cu`: what the
// occupancy query says a CU holds of the split kernel -- registers, the LDS records plus the staged sigma-point set; 0: unknown, taken
// as 4; at most 8 count), each with at least split.min_tiles tiles, none of them empty.  {1, 0}: one wave per trial.
struct WalkSegments { int segs, tiles_per_seg; };
inline WalkSegments walk_segments(WalkSplit split, int64_t B, int64_t T, int num_cus, int blocks_per_cu) {
    if (split.cap == 1) return {1, 0};
    const int64_t tiles = (T - 1 + 63) / 64;
    int64_t per_cu = blocks_per_cu > 0 ? blocks_per_cu : 4;
    if (per_cu > 8) per_cu = 8;
    int64_t segs = ((int64_t)num_cus * per_cu) / (B > 0 ? B : 1);
    if (split.cap > 1 && segs > split.cap) segs = split.cap;
    const int64_t min_tiles = split.min_tiles > 0 ? split.min_tiles : 1;
    if (segs > tiles / min_tiles) segs = tiles / min_tiles;
    if (segs > 64) segs = 64;
    if (segs < 2) return {1, 0};
    const int64_t tiles_per_seg = (tiles + segs - 1) / segs;
    return {(int)((tiles + tiles_per_seg - 1) / tiles_per_seg), (int)tiles_per_seg};      // no empty segments
}

inline WaveCandidate<SmootherRoute> smoother_wave_candidate(const SmootherQuery& q) {
    const cgp_model& m = *q.model;
    const ModelArgs& ma = *q.ma;
    const int64_t T = q.io->T;
    const bool sig = q.method == CGP_S_SGP || q.method == CGP_S_CD_SGP;
    const bool affine = (q.method == CGP_S_EKS || q.method == CGP_S_SGP) && !(q.flags & CGP_SEQUENTIAL_SCAN);
    const ShapeLimit generic = affine ? ShapeLimit{16, 1} : (sig ? ShapeLimit{8, 1} : ShapeLimit{5, 2});
    WaveCandidate<SmootherRoute> c{SmootherRoute::kNone, generic, generic};
    const bool spec = !(q.flags & CGP_GENERIC_KERNEL), mfma = !(q.flags & CGP_DPP_KERNEL);
    auto walk = [&c](SmootherRoute r, ShapeLimit against_lane4) { c.route = r; c.limit = kWaveAlways; c.limit_lane4 = against_lane4; };
    switch (m.model_id) {
    case CGP_M_LINEAR:
        c.route = SmootherRoute::kDiscLinear;
        // 5 <= d <= 8: maps built per lane, applied cooperatively in the tile layout (cgp_coop8.hpp)
        if (affine && spec && coop8_smoother_ok(m.d, T, ma)) walk(SmootherRoute::kCoop8Linear, kWaveAlways);
        // d = 4: gains per lane, the recursion walked on the matrix cores (cgp_walk4.hpp)
        else if (affine && spec && m.d == 4 && walk4_smoother_ok(T, ma)) walk(SmootherRoute::kWalk4Linear, kWaveAlways);
        break;
    case CGP_M_HARMONIC_LCD:
    case CGP_M_LASCALA_LCD:
        c.route = SmootherRoute::kDiscHarm;
        if (affine && spec && m.n_harm >= 2 && coop8_smoother_ok(m.d, T, ma) && coop8_smoother_harm_ok(q.method, ma)) walk(SmootherRoute::kCoop8Harm, kWaveAlways);
        else if (affine && spec && m.n_harm == 1 && walk4_smoother_ok(T, ma)) walk(SmootherRoute::kWalk4Harm, ShapeLimit{24, 1});
        break;
    case CGP_M_LINEAR_SDE: c.route = SmootherRoute::kSdeLinear; break;
    case CGP_M_HARMONIC_SDE: {
        // (kept as found, as for the filters: the crossovers go with the family and CGP_DPP_KERNEL, not with the kernel)
        const bool sde4 = spec && m.n_harm == 1;
        c.route = SmootherRoute::kSdeHarm;
        if (q.method == CGP_S_CD_SGP && sde4) {
            c.route = (mfma && sgp4_mfma_fits(T, ma)) ? SmootherRoute::kCdSgp4Mfma : SmootherRoute::kCdSgp4Coop;
            if (mfma) c.crossover(48, 48);
        } else if (q.method == CGP_S_CD_EKS && sde4) {
            c.route = (mfma && mfma4_rows_fit(T)) ? SmootherRoute::kCdEks4Mfma : SmootherRoute::kCdEks4Coop;
            if (mfma) c.crossover(5, 3);
        }
        break;
    }
    default: break;
    }
    return c;
}
inline SmootherRoute smoother_lane_candidate(const SmootherQuery& q) {
    const cgp_model& m = *q.model;
    const bool lane4 = m.n_harm == 1 && !(q.flags & CGP_GENERIC_KERNEL) && lane4_smoother_fits(*q.io);
    switch (m.model_id) {
    case CGP_M_LINEAR: return SmootherRoute::kDiscLinear;
    case CGP_M_HARMONIC_LCD:
    case CGP_M_LASCALA_LCD: return (q.method == CGP_S_EKS && lane4) ? SmootherRoute::kLane4 : SmootherRoute::kDiscHarm;
    case CGP_M_LINEAR_SDE: return SmootherRoute::kSdeLinear;
    case CGP_M_HARMONIC_SDE: return (q.method == CGP_S_CD_EKS && lane4) ? SmootherRoute::kLane4 : SmootherRoute::kSdeHarm;
    default: return SmootherRoute::kNone;
    }
}
inline SmootherDecision route_smoother(const SmootherQuery& q) {
    const bool sig = q.method == CGP_S_SGP || q.method == CGP_S_CD_SGP;
    const WaveCandidate<SmootherRoute> wave = smoother_wave_candidate(q);
    const SmootherRoute lane = smoother_lane_candidate(q);
    const ShapeLimit limit = lane == SmootherRoute::kLane4 ? wave.limit_lane4 : wave.limit;
    SmootherDecision d;
    auto refuse = [&d](int rc, const char* message) { d.rc = rc; d.message = message; return d; };
    d.wave = choose_wave(q.num_cus, q.io->B, q.flags, limit, sig ? q.sigma : nullptr);
    d.route = d.wave ? wave.route : lane;
    d.substeps = (q.flags & CGP_RK4_SUBSTEPS_MASK) != 0;
    if (d.substeps) {
        if (q.method != CGP_S_CD_EKS && q.method != CGP_S_CD_SGP) return refuse(CGP_E_ARG, kSubstepsDiscrete);
        if (q.segments > 1) return refuse(CGP_E_UNSUPPORTED, kSubstepsSplit);
        if (q.flags & CGP_THREAD_PER_TRIAL)
            return refuse(CGP_E_UNSUPPORTED, "CGP_RK4_SUBSTEPS: a smoother keeps the intermediate moments of an interval in LDS and runs one wavefront per trial only");
        if (sig && SigmaSet::stage_bytes(q.sigma->s, q.sigma->d, q.sigma->n_groups, q.sigma->group_start != nullptr) + substep_table_bytes(q.model->d) >
                       (size_t)kSigLdsMaxBytes)
            return refuse(CGP_E_UNSUPPORTED, "CGP_RK4_SUBSTEPS: the sigma-point set does not fit the LDS stage beside the table of intermediate moments");
        d.wave = true;
        d.route = q.model->model_id == CGP_M_LINEAR_SDE ? SmootherRoute::kSdeLinear : SmootherRoute::kSdeHarm;
    }
    d.timed = q.timed;
    if (d.timed) {
        const int id = q.model->model_id;
        if ((q.method != CGP_S_CD_EKS && q.method != CGP_S_CD_SGP) || (id != CGP_M_LINEAR_SDE && id != CGP_M_HARMONIC_SDE)) return refuse(CGP_E_ARG, kTimedDiscrete);
        if (q.segments > 1) return refuse(CGP_E_UNSUPPORTED, kTimedSplit);
        if (!honours_times(d.route)) d.route = id == CGP_M_LINEAR_SDE ? SmootherRoute::kSdeLinear : SmootherRoute::kSdeHarm;
    }
    if (q.want_sel) {
        if (writes_selection(d.route)) d.select = SmootherSelect::kKernel;
        else if (q.null_rows)
            return refuse(CGP_E_UNSUPPORTED, "this (method, model, launch shape) writes selected outputs from its full rows only: pass mss and Pss as well");
        else d.select = SmootherSelect::kGather;
    }
    // ---- time-split with burn-in (cgp_smoother_time_split): the continuous-discrete smoothers on the d = 4 matrix-core kernels, segments of
    // whole 64-step chunks; a record of one chunk, or one that leaves a single segment, is not split
    if (q.segments > 1) {
        if (q.burn_in < 0) return refuse(CGP_E_ARG, "burn_in must be >= 0");
        if (q.want_sel) return refuse(CGP_E_UNSUPPORTED, "cgp_smoother_time_split writes full rows only");
        if (!knows_segments(d.route))
            return refuse(CGP_E_UNSUPPORTED, "time-split smoothers with burn-in are built for cd_eks and cd_sgp_smoother on the d = 4 chirp / La Scala SDE (matrix-core "
                                             "kernels; standard sigma set); the discrete smoothers split exactly (CGP_TIME_SPLIT)");
        const int64_t chunks = (q.io->T - 1 + 63) / 64;
        if (chunks >= 2) {
            const int64_t cps = (chunks + q.segments - 1) / q.segments;
            const int64_t segs = (chunks + cps - 1) / cps;
            if (segs > 1) { d.bsegs = (int)segs; d.chunks_per_bseg = (int)cps; d.burn_chunks = (int)((q.burn_in + 63) / 64); }
        }
    }
    if (splits_exactly(d.route)) d.split = walk_split_policy(*q.model, q.flags, q.io->B, q.num_cus, q.walk_cap);
    return d;
}

}  // namespace cgp
#endif                         // __HIPCC_RTC__
