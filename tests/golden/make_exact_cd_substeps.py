"""Generates tests/golden/exact_cd_substeps.npz: the continuous-discrete MLE objective with n RK4 substeps between two measurements
(CGP_RK4_SUBSTEPS, include/chirpgp_hip.h) and its exact gradient in 100-digit arithmetic.  tests/test_gpu_substeps.py runs
cgp_cd_ekf_nll_grad and mle.value_and_grad against it.

Nothing is restated: n substeps ARE the filter of make_exact_cd_grad.py (nll_prefixes with skip, through its _job, evaluate and movement) at
step dt / n -- the float64 quotient, as the kernels take it -- on the record refined n times with NaN at the inserted times; a NaN of the
caller's own record is one more gap.  Admission is that file's rule: finite with a positive-definite filtering covariance at every
(refined) step, and value and gradient recomputed with every measurement and every theta moved by 1e-15 of itself move by less than 1e-13
relative and 1e-10 of the gradient's largest component.  Every case is fixed: one that fails stops the script.

Cases (records: make_exact_cd_grad.py's two, cut short): both builders, n = 2, 3, 4, T <= 40, dt = 1e-3 and 1e-2, one with gaps of its own
(at the first step and in a run), one with a non-unit H.

Entries per case `name`: .theta .params .ys (the caller's T samples) .dt (the caller's) .n .Xi .H .build .nll .grad .skip (1: the record
has NaN samples of its own, to be run with CGP_SKIP_MISSING as well) .moved_nll .moved_grad; and names, digits.

    python -m tests.golden.make_exact_cd_substeps [--procs N]      (CPU only; about 20 seconds on 8 cores)
"""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp

from tests.golden.make_exact_cd_grad import cd_case, evaluate, movement, with_nan
from tests.golden.make_exact_grad_cases import GRAD_MOVE_MAX, INIT, LASCALA_INIT, VALUE_MOVE_MAX, g_inv64, save_npz, track_record

OUT = os.path.dirname(os.path.abspath(__file__))
mp.dps = 100


def refine(ys, n):
    out = np.full(n * len(ys), np.nan)
    out[n - 1::n] = ys
    return out


def substeps_case(name, build, theta, ys, Xi, dt, n, seed, **kw):
    """The case make_exact_cd_grad.py evaluates -- the refined record at dt / n with gaps -- carrying what the caller passes beside it."""
    c = cd_case(name, 'substeps', build, theta, refine(ys, n), Xi, dt / n, seed, skip=True, **kw)
    c.update(n=n, ys_coarse=np.array(ys, dtype=np.float64), dt_coarse=dt, own_gaps=bool(np.isnan(ys).any()))
    return c


def cases():
    rng = np.random.default_rng(434343)                                  # make_exact_cd_grad.py: fixed_cases
    ys130 = track_record(rng, 130, 1e-3, 0.1, 7.0, 9.0)
    ys130_l = track_record(rng, 130, 1e-2, 0.1, 6.5, 7.5)
    th, th_l = g_inv64(INIT), g_inv64(LASCALA_INIT)
    H = np.random.default_rng(525252).uniform(-1.5, 1.5, size=4)
    return [substeps_case('sub_chirp_n2', 'chirp', th, ys130[:40], 0.1, 1e-3, 2, 300),
            substeps_case('sub_chirp_n3_H', 'chirp', th, ys130[:30], 0.1, 1e-3, 3, 301, H=H),
            substeps_case('sub_chirp_n4_gaps', 'chirp', th, with_nan(with_nan(ys130[:32], [0]), slice(5, 9)), 0.1, 1e-3, 4, 302),
            substeps_case('sub_lascala_n2', 'lascala', th_l, ys130_l[:40], 0.1, 1e-2, 2, 303),
            substeps_case('sub_lascala_n4', 'lascala', th_l, ys130_l[:24], 0.1, 1e-2, 4, 304),
            substeps_case('sub_lascala_n3_gaps', 'lascala', th_l, with_nan(ys130_l[:30], slice(14, 20)), 0.1, 1e-2, 3, 305)]


def main():
    procs = int(sys.argv[sys.argv.index('--procs') + 1]) if '--procs' in sys.argv else min(8, os.cpu_count() or 1)
    todo = cases()
    with Pool(procs) as pool:
        exact, moved = evaluate(pool, todo, False), evaluate(pool, todo, True)
    out = {'names': np.array([c['name'] for c in todo]), 'digits': mp.dps}
    for c in todo:
        n = c['name']
        e, m = exact[n], moved[n]
        dv, dg = movement(e, m) if e[2] and m[2] else (math.inf, math.inf)
        print(f"{n}: n = {c['n']}, T {len(c['ys_coarse'])}, finite and PD {e[2]}, moved {dv:.2e} / {dg:.2e}", flush=True)
        if not (e[2] and dv < VALUE_MOVE_MAX and dg < GRAD_MOVE_MAX):
            raise SystemExit(f'{n}: not admitted')
        with np.errstate(over='ignore'):
            params = np.log(np.exp(c['theta']) + 1.)
        out.update({f'{n}.theta': c['theta'], f'{n}.params': params, f'{n}.ys': c['ys_coarse'], f'{n}.dt': c['dt_coarse'], f'{n}.n': c['n'],
                    f'{n}.Xi': c['Xi'], f'{n}.H': np.array([0., 1., 0., 0.]) if c['H'] is None else c['H'], f'{n}.build': c['build'],
                    f'{n}.nll': float(e[0][-1]), f'{n}.grad': np.array([float(r[-1]) for r in e[1]]), f'{n}.skip': int(c['own_gaps']),
                    f'{n}.moved_nll': dv, f'{n}.moved_grad': dg})
    save_npz(os.path.join(OUT, 'exact_cd_substeps.npz'), out)


if __name__ == '__main__':
    main()
