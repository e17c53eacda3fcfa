"""Timing of cgp_pcrlb_sums at the Monte-Carlo size of the CRLB jobs, with cgp_squared_error_sums on the same xs as the yardstick (that
kernel reads a and r: twice the bytes, no arithmetic to speak of).

    python tools/pcrlb_probe.py [--B 262144] [--T 500] [--reps 10] [--models chirp,nh3,lin4,lin8]

Prints, per model: the median time of `reps` launches between device events (after 3 warm-up launches), the read rate it implies with
bytes = 8 d (B T + B), and the yardstick's time and rate on 16 d B T bytes.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chirpgp_amd import _engine as E, crlb, models as M, tools           # noqa: E402


def timed(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(times)), float(np.min(times))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=262144)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--models', default='chirp,nh3,lin4,lin8')
    args = ap.parse_args(argv)
    B, T, dt = args.B, args.T, 0.01
    for name in args.models.split(','):
        if name.startswith('lin'):
            d = int(name[3:])
            spec = M.linear_cond_m_cov(0.9 * np.eye(d), 0.1 * np.eye(d))
            m0, P0, H = np.zeros(d), np.eye(d), np.eye(d)[0]
        else:
            nh = {'chirp': 1, 'nh2': 2, 'nh3': 3}[name]
            d = 2 * nh + 2
            spec = M.disc_harmonic_chirp_lcd(0.1, 0.1, 1., 1., nh, 1.)
            _, _, m0, P0, H = M.model_harmonic_chirp(0.1, 0.1, 1., 1., 0.1, nh, 1.)
        xs, _ = tools.simulate_measurements(spec, H, 0.1, m0, P0, dt, T, 1, batch=B)
        x0 = tools.simulate_initial(m0, P0, 1, B)
        sums = torch.zeros((E.pcrlb_rows(d), T), dtype=torch.float64, device='cuda')
        med, best = timed(lambda: crlb.sums(spec, dt, x0, xs, sums=sums), args.reps)
        nbytes = 8 * d * (B * T + B)
        err = torch.zeros((1, 2, T), dtype=torch.float64, device='cuda')
        other = xs.clone()                                                # a second array: the yardstick reads a AND r
        ymed, ybest = timed(lambda: E.squared_error_sums(xs, other, (d - 2,), err), args.reps)
        print(f'{name:6s} d = {d}  {B} x {T}:  cgp_pcrlb_sums {med * 1e3:8.3f} ms (best {best * 1e3:.3f})  {nbytes / med / 1e12:6.2f} TB/s read   |   '
              f'cgp_squared_error_sums {ymed * 1e3:8.3f} ms (best {ybest * 1e3:.3f})  {2 * 8 * d * B * T / ymed / 1e12:6.2f} TB/s', flush=True)
        del xs, x0, other


if __name__ == '__main__':
    main()
