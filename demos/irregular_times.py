"""A chirp observed at jittered times: cd_ekf + cd_eks with the record's own time stamps (dts=) against the same samples pushed through the
plain call at the mean period.

    python demos/irregular_times.py [--T 3000] [--seed 555] [--jitter 0.75] [--out results.npz]

The samples are taken at t_k = t_{k-1} + dt (1 + jitter u_k), u uniform in (-1, 1): nothing is resampled.  tools.intervals turns the time
stamps into the per-step intervals the continuous-discrete methods integrate over; the plain call has to pretend the samples sit on a grid
of the mean period.  Prints the RMSE of the smoothed frequency estimate g(V) of both against the true frequency at the true times."""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chirpgp_amd import filters_smoothers as fs                                       # noqa: E402
from chirpgp_amd.models import build_chirp_model, g                                   # noqa: E402
from chirpgp_amd.toymodels import gen_chirp, meow_freq, constant_mag                   # noqa: E402
from chirpgp_amd.tools import intervals, rmse                                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=3000)
    ap.add_argument('--seed', type=int, default=555)
    ap.add_argument('--jitter', type=float, default=0.75)
    ap.add_argument('--out', default=None, help='write both estimates, the time stamps and the two RMSE figures to this .npz file')
    args = ap.parse_args()

    dt, T, Xi = 0.001, args.T, 0.1
    rng = np.random.default_rng(args.seed)
    ts = np.cumsum(dt * (1.0 + args.jitter * rng.uniform(-1.0, 1.0, T)))
    true_freq_func, true_phase_func = meow_freq(offset=8.)
    ys = gen_chirp(ts, constant_mag(1.), true_phase_func) + math.sqrt(Xi) * rng.standard_normal(T)
    drift, disp, _, m0, P0, H = build_chirp_model(np.array([0.1, 0.1, 0.1, 1., 1., 7.]))

    dts = intervals(ts, t0=0.0)
    mf, Pf, nll = fs.cd_ekf(drift, disp, H, Xi, m0, P0, None, ys, dts=dts)
    ms, _ = fs.cd_eks(drift, disp, mf, Pf, None, dts=dts)
    mean_dt = float(ts[-1] / T)
    mf_g, Pf_g, nll_g = fs.cd_ekf(drift, disp, H, Xi, m0, P0, mean_dt, ys)
    ms_g, _ = fs.cd_eks(drift, disp, mf_g, Pf_g, mean_dt)

    truth = true_freq_func(ts)
    err_timed, err_grid = rmse(g(ms[:, 2]), truth), rmse(g(ms_g[:, 2]), truth)
    print(f'T = {T}, dt = {dt} (1 +- {args.jitter}): intervals from {dts.min():.2e} to {dts.max():.2e} s')
    print(f'frequency RMSE with the time stamps (dts=):  {err_timed:.4f} Hz   (NLL {nll[-1]:.2f})')
    print(f'frequency RMSE at the mean period {mean_dt:.3e}: {err_grid:.4f} Hz   (NLL {nll_g[-1]:.2f})')
    if args.out:
        np.savez(args.out, ts=ts, freq_timed=g(ms[:, 2]), freq_grid=g(ms_g[:, 2]), truth=truth, rmse_timed=err_timed, rmse_grid=err_grid)


if __name__ == '__main__':
    main()
