"""What CGP_SKIP_MISSING costs in the four tangent entry points -- cgp_ekf_nll_grad, cgp_ekf_nll_fisher, cgp_sgp_nll_grad, cgp_sgp_nll_fisher --
by device events, at the shape of tests/test_gpu_fisher.py's perf test: 1500 records x T = 3141, six directions.

    python tools/gaps_grad_probe.py [--reps 7] [--R 1500] [--T 3141] [--sigma gh3|cubature] [--unflagged-only] [--out FILE]      ->  one JSON line

Per entry point: unflagged | flagged without gaps | flagged with 10 % of the samples missing in runs of 1 - 100.  The C entry points are called
directly on buffers that stay on the device, so a time is the kernel's.  Every variant is launched once to warm up; the timed launches of the
variants of one entry point ALTERNATE (a box shared with other work drifts), each between two device events; reported: the median and the
spread (min, max) in ms.  --unflagged-only times the unflagged calls alone: the same probe on a checkout whose entry points ignore the
flags word gives the figures to hold the unflagged kernels to."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench                                                                            # noqa: E402
from chirpgp_amd import _engine as E, mle                                               # noqa: E402
from chirpgp_amd import models as pm                                                    # noqa: E402
from chirpgp_amd.quadratures import SigmaPoints                                         # noqa: E402
from tools.gaps_probe import timed, with_runs_missing                                   # noqa: E402

SKIP_MISSING = 0x2000      # include/chirpgp_hip.h: CGP_SKIP_MISSING
INIT = np.array([0.1, 0.1, 0.1, 1., 1., 7.])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--R', type=int, default=1500)
    ap.add_argument('--T', type=int, default=3141)
    ap.add_argument('--sigma', choices=('gh3', 'cubature'), default='gh3')
    ap.add_argument('--unflagged-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('gaps_grad_probe: no GPU -- a time is measured on the device or not at all')
    dt, Xi, R, T = 1e-3, 0.1, args.R, args.T
    ys = bench.chirp_batch(R, T, 5, Xi=Xi)
    records = {'none': E.dev(ys)}
    if not args.unflagged_only:
        records['10pct'] = E.dev(with_runs_missing(ys, 0.10, np.random.default_rng(2024)))
    thetas = np.tile(pm.g_inv(INIT), (R, 1))
    dirs = E.dev(mle.tangent_directions(pm.build_chirp_model, thetas, dt, Xi))
    drift, disp, disc, m0, P0, H = pm.build_chirp_model(pm.g(thetas))
    lib, ctx, keep = E.load_library(), E.context(), []
    model, init = E._model_struct(disc, None, R, keep), E._init_struct(H, Xi, m0, P0, 4, R, keep)
    sg = SigmaPoints.gauss_hermite(4, 3) if args.sigma == 'gh3' else SigmaPoints.cubature(4)
    sigma = E._sigma_struct(sg, 4, keep, None)
    opts = dict(dtype=torch.float64, device='cuda')
    nll, grad, F = torch.empty((R,), **opts), torch.empty((R, 6), **opts), torch.empty((R, 6, 6), **opts)

    def launcher(entry, rec, flags):
        head = [ctx, C.byref(model)] + ([C.byref(sigma)] if '_sgp_' in entry else []) + [C.byref(init), dt, records[rec].data_ptr(), T, 1, None, R, T,
                                                                                       dirs.data_ptr(), 6, nll.data_ptr(), grad.data_ptr()]
        tail = ([F.data_ptr()] if entry.endswith('_fisher') else []) + [flags, E._stream()]
        fn = getattr(lib, entry)

        def launch():
            rc = fn(*head, *tail)
            assert rc == 0, (entry, rc, lib.cgp_last_error(ctx))
        return launch

    res = {'what': 'CGP_SKIP_MISSING in the tangent entry points: kernel times in ms (median of alternating launches, device events)',
           'R': R, 'T': T, 'n_dir': 6, 'sigma': args.sigma, 'reps': args.reps, 'source_hash': E.source_hash()[:16], 'table': {}}
    for entry in ('cgp_ekf_nll_grad', 'cgp_ekf_nll_fisher', 'cgp_sgp_nll_grad', 'cgp_sgp_nll_fisher'):
        variants = {'unflagged': launcher(entry, 'none', 0)}
        if not args.unflagged_only:
            variants['flagged_no_gaps'] = launcher(entry, 'none', SKIP_MISSING)
            variants['flagged_10pct_missing'] = launcher(entry, '10pct', SKIP_MISSING)
        res['table'][entry] = timed(variants, args.reps)
        torch.cuda.synchronize()
        assert np.isfinite(nll.cpu().numpy()).all(), entry                  # (the last launch of the entry point: every trial finite)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
