"""HIP-event time of cgp_smoother_sample (posterior sample paths, csrc/cgp_sample4.hpp) and the output rate it reaches.

    python tools/sample_probe.py [--B 1000] [--T 10000] [--S 64] [--launches 20] [--warmup 3] [--normals]

Cases: the large batch B x T x S with comp_paths only (8 B a sample-step) and with paths as well (40 B), and one record 1 x 3141 x 1024.
B is halved until inputs and outputs fit the card's free memory.  The median of the launches is printed beside the output bytes/s; the
large-batch smoothers write 4.6 - 5.0 TB/s (README.md).  One JSON line per case."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    import torch
    from chirpgp_amd import filters_smoothers as fs
    from chirpgp_amd.models import build_chirp_model
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=1000)
    ap.add_argument('--T', type=int, default=10000)
    ap.add_argument('--S', type=int, default=64)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args(argv)
    dt, Xi = 1e-3, 0.1
    _, _, cond, m0, P0, H = build_chirp_model(np.array([0.1, 0.1, 0.1, 1., 1., 7.]))
    results = []

    def case(label, B, T, S, want_paths):
        per_step = 8 * (1 + (4 if want_paths else 0))
        need = lambda b: b * S * T * per_step + b * T * 8 * 21          # noqa: E731  (outputs + filtering rows + measurements)
        free, _ = torch.cuda.mem_get_info()
        while B > 1 and need(B) > 0.8 * free:
            B //= 2
        ts = dt * np.arange(1, T + 1)
        ys = torch.as_tensor(np.sin(2 * np.pi * 8. * ts)[None] + 0.3 * np.random.default_rng(0).standard_normal((B, T))).cuda()
        mfs, Pfs, _ = fs.ekf(cond, H, Xi, m0, P0, dt, ys)
        del ys
        times = []
        for i in range(args.warmup + args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fs.eks_sample(cond, mfs, Pfs, dt, S, seed=i, want_paths=want_paths, select=dict(comp=2, func='softplus'))
            e1.record()
            torch.cuda.synchronize()
            del out
            if i >= args.warmup:
                times.append(e0.elapsed_time(e1))
        ms = statistics.median(times)
        r = dict(case=label, B=B, T=T, S=S, paths=want_paths, ms_median=round(ms, 3), ms_min=round(min(times), 3), launches=len(times),
                 output_GB=round(B * S * T * per_step / 1e9, 3), output_TB_per_s=round(B * S * T * per_step / ms / 1e9, 3),
                 sample_steps_per_s=round(B * S * T / ms * 1e3, 0), smoothers_TB_per_s='4.6 - 5.0')
        print(json.dumps(r), flush=True)
        results.append(r)
        del mfs, Pfs
        torch.cuda.empty_cache()

    case('batch, comp_paths only', args.B, args.T, args.S, False)
    case('batch, paths + comp_paths', args.B, args.T, args.S, True)
    case('one record, comp_paths only', 1, 3141, 1024, False)
    case('one record, paths + comp_paths', 1, 3141, 1024, True)
    return results


if __name__ == '__main__':
    main()
