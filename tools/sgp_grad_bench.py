"""Sigma-point filter objective: exact gradient (cgp_sgp_nll_grad, forward tangents) against the 13-probe central difference -- time per
objective evaluation at T = 3141 for R = 1, 64 and 1000 records in one launch, and one fit on the demo's record (demos/ghfs_mle.py).
python tools/sgp_grad_bench.py [--sigma gh3|cubature] [--profile]   (--profile: five exact evaluations at R = 64 only, for rocprofv3)"""
import hashlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chirpgp_amd import _engine as E, mle, models as pm                    # noqa: E402
from chirpgp_amd.quadratures import SigmaPoints                            # noqa: E402
from tools.grad_bench import INIT, record                                  # noqa: E402


def _library_sha256():
    with open(os.path.join(os.path.dirname(E.__file__), 'libchirpgp_hip.so'), 'rb') as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    name = sys.argv[sys.argv.index('--sigma') + 1] if '--sigma' in sys.argv else 'gh3'
    sg = SigmaPoints.gauss_hermite(4, 3) if name == 'gh3' else SigmaPoints.cubature(4)
    E.load_library()
    print(f'libchirpgp_hip.so sha256 {_library_sha256()}, sources {E.source_hash()[:16]}; {torch.cuda.get_device_name(0)}; '
          f'sigma set {name} ({sg.n_points} points)', flush=True)
    th = pm.g_inv(INIT)
    ys = record(3141, 555)
    if '--profile' in sys.argv:
        recs = torch.from_numpy(np.stack([record(3141, 1000 + r) for r in range(64)])).cuda()
        for _ in range(5):
            mle._value_and_grad_many('sgp_filter', pm.build_chirp_model, np.tile(th, (64, 1)), recs, 0.1, 1e-3, sg, 1e-6, {}, exact=True)
        torch.cuda.synchronize()
        return
    for R in (1, 64, 1000):
        recs = np.stack([record(3141, 1000 + r) for r in range(R)]) if R > 1 else ys[None, :]
        yd = torch.from_numpy(recs).cuda()
        ths = np.tile(th, (R, 1))
        for exact in (True, False):
            args = ('sgp_filter', pm.build_chirp_model, ths, yd, 0.1, 1e-3, sg, 1e-6, {})
            mle._value_and_grad_many(*args, exact=exact)
            torch.cuda.synchronize()
            n = 10 if R < 1000 else 3
            t0 = time.perf_counter()
            for _ in range(n):
                mle._value_and_grad_many(*args, exact=exact)
            torch.cuda.synchronize()
            form = 'exact (tangent kernel)' if exact else '13-probe differences'
            print(f'R = {R:4d} records, T = 3141, {form:22s}: {(time.perf_counter() - t0) / n * 1e3:8.2f} ms per value + gradient of all records',
                  flush=True)
    for exact in (True, False):
        t0 = time.perf_counter()
        opt, res = mle.fit('sgp_filter', pm.build_chirp_model, INIT, ys, 0.1, 1e-3, sgps=sg, maxiter=300, exact=exact)
        print(f'fit on the demo record, exact = {exact}: {time.perf_counter() - t0:.2f} s ({res.nit} iterations, {res.nfev} evaluations, '
              f'nll {res.fun:.9f}, params {np.array2string(opt, precision=5)})', flush=True)


if __name__ == '__main__':
    main()
