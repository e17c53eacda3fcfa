"""What the exact gradient of the cd_sgp_filter objective costs beside the difference gradient it replaces on request: one launch of
cgp_sgp_nll_grad on the SDE model (R records, one wavefront each, 6 directions) against one 13-probe difference launch (R x 13 filter
passes of cd_sgp_filter) -- the route of mle.make_objective('cd_sgp_filter', exact=False) -- at T = 3141 for R = 1, 64 and 1000 records,
with Gauss-Hermite order 3 (81 points) and the cubature rule (8).

    python tools/cd_sgp_grad_probe.py [--reps 7] [--T 3141] [--R 1 64 1000] [--sets gh3 cubature] [--out FILE]      ->  one JSON line

Per set and R three times in ms, median of `reps` alternating launches between device events after a warm-up launch of each
(tools/gaps_probe.py: timed), with the fastest and the slowest:
    exact_kernel   the C entry point on buffers that stay on the device: the kernel's own time
    exact_call     mle.value_and_grad(method='cd_sgp_filter') on the device-resident records: the kernel and the host's directions and marshalling
    difference     the 13-probe launch through mle.batched_nll, as make_objective / fit_many issue it: kernel and marshalling
and the difference gradient's distance from the exact one, of the gradient's scale.  No default depends on these numbers; they are
measured, not gated.  Run it under a time limit of its own."""
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
from tools.gaps_probe import timed                                                      # noqa: E402

INIT = np.array([0.1, 0.1, 0.1, 1., 1., 7.])
SETS = {'gh3': lambda: SigmaPoints.gauss_hermite(4, 3), 'cubature': lambda: SigmaPoints.cubature(4), 'gh4': lambda: SigmaPoints.gauss_hermite(4, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--T', type=int, default=3141)
    ap.add_argument('--R', type=int, nargs='+', default=[1, 64, 1000])
    ap.add_argument('--sets', nargs='+', default=['gh3', 'cubature'], choices=sorted(SETS))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('cd_sgp_grad_probe: no GPU -- a time is measured on the device or not at all')
    dt, Xi, T, P = 1e-3, 0.1, args.T, 6
    lib, ctx = E.load_library(), E.context()
    res = {'what': 'cd_sgp_filter objective and gradient: exact (cgp_sgp_nll_grad on the SDE model) against 13-probe differences, ms (median of alternating '
                   'launches, device events)', 'T': T, 'n_dir': P, 'reps': args.reps, 'source_hash': E.source_hash()[:16], 'table': {}}
    for name in args.sets:
        sg = SETS[name]()
        for R in args.R:
            ys = E.dev(bench.chirp_batch(R, T, 5, Xi=Xi))
            thetas = np.tile(pm.g_inv(INIT), (R, 1))
            # ---- the entry point itself
            keep = []
            drift, disp, _, m0, P0, H = pm.build_chirp_model(pm.g(thetas))
            model, init = E._model_struct(drift, disp.outer(), R, keep), E._init_struct(H, Xi, m0, P0, 4, R, keep)
            sig = E._sigma_struct(sg, 4, keep, None)
            dirs = E.dev(mle.tangent_directions_cd(pm.build_chirp_model, thetas, dt, Xi))
            opts = dict(dtype=torch.float64, device='cuda')
            nll, grad = torch.empty((R,), **opts), torch.empty((R, P), **opts)

            def exact_kernel():
                rc = lib.cgp_sgp_nll_grad(ctx, C.byref(model), C.byref(sig), C.byref(init), dt, ys.data_ptr(), T, 1, None, R, T, dirs.data_ptr(), P, nll.data_ptr(),
                                          grad.data_ptr(), 0, E._stream())
                assert rc == 0, (rc, lib.cgp_last_error(ctx))

            # ---- the two routes as mle issues them
            h = 1e-6 * (1.0 + np.abs(thetas))
            batch = np.repeat(thetas[:, None, :], 2 * P + 1, axis=1)
            idx = np.arange(P)
            batch[:, 1 + 2 * idx, idx] += h
            batch[:, 2 + 2 * idx, idx] -= h
            batch = batch.reshape(-1, P)
            out = {}

            def exact_call():
                out['exact'] = mle.value_and_grad(pm.build_chirp_model, thetas, ys, Xi, dt, method='cd_sgp_filter', sgps=sg)

            def difference():
                out['diff'] = mle.batched_nll('cd_sgp_filter', pm.build_chirp_model, batch, ys, Xi, dt, sg)

            row = timed({'exact_kernel': exact_kernel, 'exact_call': exact_call, 'difference': difference}, args.reps)
            torch.cuda.synchronize()
            f, g_ = out['exact']
            nd = out['diff'].reshape(R, 2 * P + 1)
            gd = (nd[:, 1::2] - nd[:, 2::2]) / (2 * h)
            assert np.isfinite(f).all() and np.array_equal(f, nll.cpu().numpy())
            row['us_per_step_exact_kernel'] = round(1e3 * row['exact_kernel']['ms'] / T, 3)
            row['difference_gradient_off_by'] = float(np.max(np.abs(gd - g_).max(axis=1) / np.abs(g_).max(axis=1)))      # of the gradient's scale
            row['value_off_by'] = float(np.max(np.abs(nd[:, 0] - f) / np.abs(f)))
            res['table'][f'{name} R={R}'] = row
            print(f'{name} R={R}: {json.dumps(row)}', file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
