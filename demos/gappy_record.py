"""A record with gaps: MLE (central differences) -> EKF -> EKS -> E[g(V)] on a toy chirp with three gaps and a tail to forecast.

    python demos/gappy_record.py [--T 3141] [--seed 555] [--maxiter 200] [--stderr] [--out results.npz]

Missing samples are NaN in the record and every filter call says missing='skip': at such a step the prediction is the filtering result
and the likelihood gains nothing, so the objective is the likelihood of the observed samples alone.  The smoother needs no keyword -- it
reads the filtering rows and predicts again -- and fills the gaps from both sides; the tail it can only forecast.  The RMSE of the
frequency estimate is printed over the observed steps and over the gaps apart.

--stderr: the estimates with their standard errors, from the Fisher information of the observed samples' innovations at the optimum (one
more launch: cgp_ekf_nll_fisher with CGP_SKIP_MISSING, mle.standard_errors(..., missing='skip')); "flat" where the information is singular.
(The tangent kernels take gaps, but mle.fit still differences the objective's gradient on a record with gaps.)"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chirpgp_amd import filters_smoothers as fs, mle                                   # noqa: E402
from chirpgp_amd.models import build_chirp_model                                      # noqa: E402
from chirpgp_amd.toymodels import gen_chirp, meow_freq, constant_mag                   # noqa: E402
from chirpgp_amd.tools import rmse                                                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=3141)
    ap.add_argument('--seed', type=int, default=555)
    ap.add_argument('--maxiter', type=int, default=200)
    ap.add_argument('--stderr', action='store_true', help='standard errors of the estimates from the observed samples\' Fisher information')
    ap.add_argument('--out', default=None, help='write the estimate, the gap mask and the two RMSE figures to this .npz file')
    args = ap.parse_args()

    dt, T, Xi = 0.001, args.T, 0.1
    ts = np.linspace(dt, dt * T, T)
    rng = np.random.default_rng(args.seed)
    true_freq_func, true_phase_func = meow_freq(offset=8.)
    ys = gen_chirp(ts, constant_mag(1.), true_phase_func) + math.sqrt(Xi) * rng.standard_normal(T)
    # three gaps -- a dropped sample, a short burst, a gated segment of 6 % of the record -- and the last 5 % to forecast
    missing = np.zeros(T, dtype=bool)
    for a, b in ((T // 10, T // 10 + 1), (T // 4, T // 4 + 25), (T // 2, T // 2 + (3 * T) // 50), (T - T // 20, T)):
        missing[a:b] = True
    ys[missing] = np.nan

    t0 = time.time()
    opt_params, res = mle.fit('ekf', build_chirp_model, [0.1, 0.1, 0.1, 1., 1., 7.], ys, Xi, dt, maxiter=args.maxiter, missing='skip')
    _, _, m_and_cov, m0, P0, H = build_chirp_model(opt_params)
    mfs, Pfs, nll = fs.ekf(m_and_cov, H, Xi, m0, P0, dt, ys, missing='skip')
    mss, Pss, sel = fs.eks(m_and_cov, mfs, Pfs, dt, select=dict(comp=2, expect='softplus'))
    est, truth = sel['expect'], true_freq_func(ts)
    rmse_obs, rmse_gap = rmse(truth[~missing], est[~missing]), rmse(truth[missing], est[missing])
    print(f'{int(missing.sum())} of {T} samples missing   params {np.array2string(opt_params, precision=3)}  nll {res.fun:.2f}  iters {res.nit} '
          f'({res.nfev} launches)  [{time.time() - t0:.2f} s]')
    print(f'RMSE of the frequency estimate: {rmse_obs:.3f} Hz over the observed steps, {rmse_gap:.3f} Hz over the gaps and the forecast tail')
    extra = {}
    if args.stderr:
        se, _, info = mle.standard_errors(build_chirp_model, res.x, ys, Xi, dt, missing='skip')
        print(f'standard errors from the information of the {T - int(missing.sum())} observed samples '
              f'(cond of the scaled information {info["cond"]:.3g}):')
        for name, p, s in zip(('lam', 'b', 'delta', 'ell', 'sigma', 'm0_v'), opt_params, se):
            print(f'  {name:6s} {p:10.4g} +- {"flat" if info["singular"] or not np.isfinite(s) else f"{s:.3g}"}')
        extra = dict(standard_errors=se, fisher=info['fisher'])      # (stored with --stderr only; inf where flat)
    if args.out:
        np.savez(args.out, estimate=est, smoothed_mean=mss, filtered_nll=nll, missing=missing.astype(np.float64), params=opt_params,
                 rmse_observed=rmse_obs, rmse_gaps=rmse_gap, **extra)


if __name__ == '__main__':
    main()
