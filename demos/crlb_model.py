"""Counterpart of the job the reference's tetralith/run_crlb_model.sh starts (jobs/crlb_model.py -lam -b -delta -ell -sigma -Xi) on the
MI355X engine: the posterior Cramer-Rao lower bound of the chirp model by Monte Carlo (chirpgp/models.py:583-644) -- the curve the
error statistics of demos/crlb_ekf.py are meant to be compared against.  Trajectories are simulated on the device (cgp_simulate,
cgp_simulate_x0), the per-sample Hessian blocks are summed over the trials per time step on the device (cgp_pcrlb_sums), and the T
solves of 4 x 4 run on the host (chirpgp_amd/crlb.py).  Nothing but K T = 26 T doubles of sums leaves HBM.

    python demos/crlb_model.py [-lam 0.1 -b 0.1 -delta 0.1 -ell 1 -sigma 1 -Xi 0.1] [--num-mcs 1000000] [--T 500] [--chunk 250000]
                               [--seed 666] [--save bound.npz] [--with-ekf]

--with-ekf also filters the same trials with the EKF and prints bound / mean squared error at three steps (a report, not a gate:
the bound is a bound on any estimator, and the EKF is not efficient).
With torch.distributed initialised (python -m torch.distributed.run --nproc-per-node N demos/crlb_model.py ...) every rank takes a
contiguous block of the trials and the sums are all-reduced once, like demos/crlb_ekf.py.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chirpgp_amd import crlb, filters_smoothers as fs, tools, _engine       # noqa: E402
from chirpgp_amd.models import model_chirp, disc_chirp_lcd                    # noqa: E402
from chirpgp_amd.parallel import shard_bounds                                 # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    for name, default in (('-lam', 0.1), ('-b', 0.1), ('-delta', 0.1), ('-ell', 1.0), ('-sigma', 1.0), ('-Xi', 0.1)):
        ap.add_argument(name, type=float, default=default)
    ap.add_argument('--num-mcs', type=int, default=1000000)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--chunk', type=int, default=250000, help='trials per launch (bounds the HBM held at once)')
    ap.add_argument('--seed', type=int, default=666)
    ap.add_argument('--save', default=None, help='write ts, js and the bound\'s diagonal entries to this .npz')
    ap.add_argument('--with-ekf', action='store_true', help='also run the EKF on the same trials and print bound / MSE at three steps')
    args = ap.parse_args(argv)

    rank, world = 0, 1
    if 'RANK' in os.environ:
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)))
        dist.init_process_group('nccl')
        rank, world = dist.get_rank(), dist.get_world_size()

    _, _, m0, P0, H = model_chirp(args.lam, args.b, args.ell, args.sigma, args.delta)
    m_and_cov = disc_chirp_lcd(args.lam, args.b, args.ell, args.sigma)
    dt, T, d = 0.01, args.T, 4
    lo, hi = shard_bounds(args.num_mcs, rank, world)
    sums = torch.zeros((_engine.pcrlb_rows(d), T), dtype=torch.float64, device='cuda')
    errs = torch.zeros((2, 2, T), dtype=torch.float64, device='cuda') if args.with_ekf else None
    # warm-up: library load, code-object load and the first allocations are one-off costs of the process
    xw, yw = tools.simulate_measurements(m_and_cov, H, args.Xi, m0, P0, dt, 8, args.seed, batch=64)
    crlb.sums(m_and_cov, dt, tools.simulate_initial(m0, P0, args.seed, 64), xw)
    if args.with_ekf:
        fs.ekf(m_and_cov, H, args.Xi, m0, P0, dt, yw, want=(True, False, False))
    torch.cuda.synchronize()
    t0 = time.time()
    for first in range(lo, hi, args.chunk):
        n = min(args.chunk, hi - first)
        xss, yss = tools.simulate_measurements(m_and_cov, H, args.Xi, m0, P0, dt, T, args.seed, batch=n, trial0=first,
                                               states=True)
        x0 = tools.simulate_initial(m0, P0, args.seed, n, trial0=first)
        crlb.sums(m_and_cov, dt, x0, xss, sums=sums)
        if args.with_ekf:
            mfs, _, _ = fs.ekf(m_and_cov, H, args.Xi, m0, P0, dt, yss, want=(True, False, False))
            _engine.squared_error_sums(mfs, xss, (1, 2), errs)
            del mfs
        del xss, yss, x0
    if world > 1:
        dist.all_reduce(sums)                                              # K T doubles
        if errs is not None:
            dist.all_reduce(errs)
    torch.cuda.synchronize()
    t1 = time.time()
    out = None
    if rank == 0:
        n = args.num_mcs
        js = crlb.recursion(sums, n, np.linalg.inv(P0), m_and_cov, H, args.Xi, dt)
        bound = crlb.bound(js)
        ts = dt * np.arange(1, T + 1)
        print(f'{n} trials x {T} steps on {world} GPU(s): simulate + Cramer-Rao sums' + (' + EKF' if args.with_ekf else '') + f' {t1 - t0:.3f} s')
        if args.save:
            np.savez(args.save, ts=ts, js=js, crlb_chirps=bound[:, 1, 1], crlb_vs=bound[:, 2, 2])
        for k in (0, T // 2, T - 1):
            line = f'  t = {ts[k]:5.2f}  bound: chirp {bound[k, 1, 1]:.4e}   v {bound[k, 2, 2]:.4e}'
            if args.with_ekf:
                mse_c, mse_v = errs[0, 0, k].item() / n, errs[1, 0, k].item() / n
                line += f'   bound / EKF MSE: chirp {bound[k, 1, 1] / mse_c:.3f}   v {bound[k, 2, 2] / mse_v:.3f}'
            print(line)
        out = ts, js, bound
    if world > 1:
        dist.destroy_process_group()
    return out


if __name__ == '__main__':
    main()
