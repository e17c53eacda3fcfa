"""What missing='skip' (CGP_SKIP_MISSING) costs, and where its launch shapes cross over: kernel times by device events on the bench's records.

    python tools/gaps_probe.py [--reps 7] [--no-crossovers] [--out FILE]      ->  one JSON line

table       B = 1000, T = 10^4 (the shape of BASELINE C2 / C3; C4's kernels at the same shape), full outputs, inputs and outputs in HBM:
            ekf and sgp_filter (GH-3) unflagged | flagged without gaps | flagged with 10 % of the samples missing in runs of 1 - 100 |
            flagged + CGP_GENERIC_KERNEL; cd_ekf and cd_sgp_filter unflagged | flagged.
crossovers  flagged ekf and sgp_filter on the chirp model at T = 500, B = 2048 .. 16 384, one wavefront against one lane per trial.

Every variant is launched once to warm up; the timed launches of the variants of one method ALTERNATE (a box shared with other work drifts),
each between two device events; reported: the median and the spread (min, max) in ms."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench                                                                            # noqa: E402
from chirpgp_amd import _engine as E, filters_smoothers as fs                           # noqa: E402
from chirpgp_amd.models import build_chirp_model                                        # noqa: E402
from chirpgp_amd.quadratures import SigmaPoints                                         # noqa: E402

WAVE, THREAD, GENERIC = 0x2, 0x4, 0x10


def with_runs_missing(ys, share, rng):
    """NaN over runs of 1 - 100 steps, placed at random until `share` of every record is missing."""
    out = np.array(ys)
    B, T = out.shape
    for b in range(B):
        missing = 0
        while missing < share * T:
            n = int(rng.integers(1, 101))
            a = int(rng.integers(0, T - n + 1))
            missing += int(np.isfinite(out[b, a:a + n]).sum())
            out[b, a:a + n] = np.nan
    return out


def timed(variants, reps):
    """variants: name -> callable that enqueues one launch.  -> name -> dict(ms, min, max)."""
    import torch
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: dict(ms=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--B', type=int, default=1000)
    ap.add_argument('--T', type=int, default=10000)
    ap.add_argument('--no-crossovers', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('gaps_probe: no GPU -- a time is measured on the device or not at all')
    dt, Xi = 1e-3, 0.1
    drift, disp, disc, m0, P0, H = build_chirp_model(np.array([0.1, 0.1, 0.1, 1., 1., 7.]))
    sg = SigmaPoints.gauss_hermite(4, 3)
    b_mat = disp(None)
    rng = np.random.default_rng(2024)

    def launchers(ys_d, flags, missing):
        kw = dict(flags=flags, missing=missing)
        return {'ekf': lambda: fs.ekf(disc, H, Xi, m0, P0, dt, ys_d, **kw),
                'sgp_filter': lambda: fs.sgp_filter(disc, sg, H, Xi, m0, P0, dt, ys_d, **kw),
                'cd_ekf': lambda: fs.cd_ekf(drift, disp, H, Xi, m0, P0, dt, ys_d, **kw),
                'cd_sgp_filter': lambda: fs.cd_sgp_filter(drift, b_mat, sg, H, Xi, m0, P0, dt, ys_d, **kw)}

    ys = bench.chirp_batch(args.B, args.T, 5, Xi=Xi)
    ys_d, gaps_d = E.dev(ys), E.dev(with_runs_missing(ys, 0.10, rng))
    res = {'what': 'missing=skip: kernel times in ms (median of alternating launches, device events)', 'B': args.B, 'T': args.T, 'reps': args.reps, 'table': {}}
    for method in ('ekf', 'sgp_filter'):
        res['table'][method] = timed({'unflagged': launchers(ys_d, 0, None)[method],
                                      'flagged_no_gaps': launchers(ys_d, 0, 'skip')[method],
                                      'flagged_10pct_missing': launchers(gaps_d, 0, 'skip')[method],
                                      'flagged_generic': launchers(ys_d, GENERIC, 'skip')[method]}, args.reps)
    for method in ('cd_ekf', 'cd_sgp_filter'):
        res['table'][method] = timed({'unflagged': launchers(ys_d, 0, None)[method], 'flagged_no_gaps': launchers(ys_d, 0, 'skip')[method]},
                                     max(3, args.reps // 2))
    if not args.no_crossovers:
        res['crossovers'] = {'T': 500, 'simds': 4 * torch.cuda.get_device_properties(0).multi_processor_count}
        for B in (2048, 4096, 8192, 16384):
            y = E.dev(bench.chirp_batch(B, 500, 5, Xi=Xi))
            for method in ('ekf', 'sgp_filter'):
                res['crossovers'][f'{method}_B{B}'] = timed({'wave': launchers(y, WAVE, 'skip')[method], 'lane': launchers(y, THREAD, 'skip')[method]}, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
