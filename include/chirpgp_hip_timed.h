/*
 * chirpgp_hip_timed.h -- the continuous-discrete methods of libchirpgp_hip.so on records with their own time stamps.
 *
 * cd_ekf, cd_eks, cd_sgp_filter and cd_sgp_smoother integrate a moment ODE between measurements, so nothing in them needs the samples on a
 * grid: cgp_filter and cgp_smoother (chirpgp_hip.h) take one dt for the whole record, the two entry points below take one interval per
 * step.  Plain C99; a header of its own, so that chirpgp_hip.h and CGP_VERSION stay what they are.
 *
 * THE DEFINITION.  dts[t], t = 0 .. T - 1, float64, is the time from sample t - 1 to sample t; dts[0] runs from the initial condition
 * (m0, P0) to sample 0 (the reference predicts over dt before its first update, and so does this).
 *   Filter, step t:        the prediction from (mf_{t-1}, Pf_{t-1}) is ONE RK4 step of length dts[t]; with CGP_RK4_SUBSTEPS(n) it is n steps
 *                          of h_t = dts[t] / n -- one correctly rounded division in the kernel, never a reciprocal approximation.  The
 *                          update is cgp_filter's.  CGP_SKIP_MISSING composes unchanged.
 *   Smoother, step t+1->t: the backward RK4 step over dts[t + 1]; with CGP_RK4_SUBSTEPS(n) cgp_smoother's substep scheme over that interval.
 *                          dts[0] is never read by a smoother.
 *   Zero interval:         dts[t] = 0 is legal and means two measurements at one instant: the RK4 step is the identity on finite moments.
 *   Bad intervals:         these entry points do not read device memory on the host.  A NaN interval poisons the state from its step on,
 *                          like a NaN measurement without CGP_SKIP_MISSING; a negative or infinite one is integrated as given.  (The Python
 *                          front ends refuse NaN, +-inf and negative entries before anything is launched.)
 *   On a constant grid, dts[t] = dt for every t, both entry points compute what cgp_filter / cgp_smoother compute with that dt.
 *
 * ADDRESSING.  The intervals belong to the record.
 *   Filters:   trial b reads dts + rec(b) * dts_stride with the rec(b) of its measurements (ys_repeat, ys_index: cgp_filter).
 *              dts_stride = 0: one time grid for the whole call; any value >= 0 is legal.  Every probe of a record in a parameter sweep
 *              reads the ONE copy of its grid, as it does of its samples.
 *   Smoothers: a smoother has no record addressing of its own, so the intervals bring theirs, with the same rule: trial b reads grid
 *              dts_index[b / dts_repeat] (b / dts_repeat without an index), dts_stride doubles apart; dts_repeat >= 1.
 *
 * ACCEPTED.  CGP_F_CD_EKF, CGP_F_CD_SGP, CGP_S_CD_EKS, CGP_S_CD_SGP on every SDE model cgp_filter / cgp_smoother take; every launch-shape
 * flag, CGP_NLL_FINAL_ONLY, CGP_SKIP_MISSING and CGP_RK4_SUBSTEPS(n), with the meaning and the refusals they have there.
 * REFUSED, nothing written, cgp_last_error names the reason:
 *   dts == NULL, dts_stride < 0, dts_repeat < 1      CGP_E_ARG
 *   a discrete method or model                        CGP_E_ARG: their constants (exp(-lam dt), the Matern-3/2 transition) are fixed per dt at set-up
 *   B == 0 or T == 0                                  CGP_OK, nothing touched
 * NOT BUILT.  There are no timed forms of the time-split entry points (cgp_filter_time_split, cgp_smoother_time_split), of
 * cgp_smoother_sample, of the tangent / Fisher entry points (cgp_*_nll_grad, cgp_*_nll_fisher) and of the run-time compiled models
 * (cgp_filter_custom, cgp_smoother_custom): those take one dt.
 */
#ifndef CHIRPGP_HIP_TIMED_H
#define CHIRPGP_HIP_TIMED_H

#include "chirpgp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CGP_TIMED_VERSION 1

/* cgp_filter with per-step intervals.  Outputs, flags and every other argument as in cgp_filter. */
int cgp_filter_timed(cgp_ctx* ctx, int method, const cgp_model* model, const cgp_sigma* sigma, const cgp_init* init,
                     const double* dts, int64_t dts_stride,
                     const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index,
                     int64_t B, int64_t T, double* mfs, double* Pfs, double* nll, uint32_t flags, void* stream);

/* cgp_smoother / cgp_smoother_select with per-step intervals: `out` as in cgp_smoother_select -- full rows (mss, Pss), selected outputs, or
 * both --, so one entry point covers both. */
int cgp_smoother_timed(cgp_ctx* ctx, int method, const cgp_model* model, const cgp_sigma* sigma,
                       const double* dts, int64_t dts_stride, int64_t dts_repeat, const int32_t* dts_index,
                       const double* mfs, const double* Pfs, int64_t B, int64_t T,
                       const cgp_smooth_out* out, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHIRPGP_HIP_TIMED_H */
