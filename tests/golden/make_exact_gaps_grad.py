"""Generates tests/golden/exact_gaps_grad.npz: the MLE objective of a record WITH GAPS -- ekf(...)[-1][-1] and sgp_filter(...)[-1][-1] with
every NaN measurement skipped (mf = mp, Pf = Pp, NLL increment 0) -- its exact gradient and the Fisher information of the OBSERVED samples'
innovations model,

    F[i][j] = sum over observed steps t of ( d nu_i d nu_j / S  +  d S_i d S_j / (2 S^2) ),

in 100-digit arithmetic.  tests/test_gpu_gaps_gradient.py runs cgp_ekf_nll_grad, cgp_sgp_nll_grad, cgp_ekf_nll_fisher and cgp_sgp_nll_fisher
with CGP_SKIP_MISSING against it; tests/test_gaps_grad_fixture.py ties its values to the float64 oracle with gaps (tests/gap_oracle.py).

Nothing is restated.  The pass over a case is make_exact_grad_cases._job -- the float64 inputs taken as exact, theta_k or Xi moved by
+-1e-30, the inputs moved by 1e-15 with seeded signs (NaN stays NaN) -- and it hands every step's predicted moments to linear_update
(filters_smoothers.py:55-68).  Here that call is wrapped, as make_exact_fisher._job wraps it: a NaN measurement returns (mp, Pp, 0) and
notes nothing; any other notes (nu_t, S_t) and calls through.  ONE set of passes gives the value, the gradient (central differences, step
1e-30) and, from the noted steps, the Fisher matrix (make_exact_fisher.fisher_prefixes over the observed steps).

Inputs are cases of tests/golden/exact_grad_cases.npz, read by name, with NaN over half-open step ranges (PATTERNS).  The cases, one line
of CASES each: the T = 130 EKF record under 14 patterns (no gap; the first / last step; a leading and a trailing run; the steps beside and
across the EKF kernel's 8-step block and the sigma-point kernel's 64-step chunk; long gaps; every odd step; `mixed`; one observed step),
`mixed` on five further EKF cases (La Scala, non-unit H with d / d Xi, lam = 0), four patterns on the T = 130 Gauss-Hermite record, two
cubature cases, one further Gauss-Hermite case.

Admission, as make_exact_grad_cases and make_exact_fisher: everything is recomputed with every measurement and every theta moved by 1e-15
of itself; the value must move by less than 1e-13 relative, the gradient by less than 1e-10 of its largest component, the matrix by less
than 1e-10 of its largest entry -- a hundredth of the gates the tests apply.  The edge_* cases are exempt and carry their movement.  A
case that fails is left out and listed under `rejected`; the file must keep at least 22 of the 26 cases and one of every line.
The pattern without a gap must reproduce prefix_ekf's stored value and gradient and exact_fisher.npz's matrix to the last digit: asserted.

Entries: names; name.source (the case of exact_grad_cases.npz) / .pattern / .gaps (n, 2: the half-open ranges) / .ys (the record with its
NaN) / .n_dir / .n_observed / .nll / .grad / .fisher / .moved_nll / .moved_grad / .moved_fisher; rejected, rejected_moved (n, 3).

    python -m tests.golden.make_exact_gaps_grad [--procs N]      (CPU only; a few minutes on 8 cores)
"""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

import tests.golden.make_exact_fisher as mf
import tests.golden.make_exact_grad_cases as mg

OUT = os.path.dirname(os.path.abspath(__file__))
mp.dps = 100
MIN_CASES = 22


def odd(T):
    return tuple((t, t + 1) for t in range(1, T, 2))


def mixed(T):
    return ((0, 1), (6, 10), (37, 38), (60, 70), (T - 3, T))


def all_but(T, keep):
    return ((0, keep), (keep + 1, T))


# pattern name -> the half-open step ranges on a record of T samples
PATTERNS = {'none': lambda T: (), 'first': lambda T: ((0, 1),), 'last': lambda T: ((T - 1, T),), 'lead9': lambda T: ((0, 9),),
            'trail10': lambda T: ((T - 10, T),), 'step7': lambda T: ((7, 8),), 'step8': lambda T: ((8, 9),), 'block6_10': lambda T: ((6, 10),),
            'chunk60_70': lambda T: ((60, 70),), 'long64_128': lambda T: ((64, 128),), 'long20_110': lambda T: ((20, 110),), 'odd': odd,
            'mixed': mixed, 'all_but_65': lambda T: all_but(T, 65)}
# one line of the list each: the fixture keeps at least one case of every line.  (source, pattern)
CASES = (tuple(('prefix_ekf', p) for p in PATTERNS),
         tuple((s, 'mixed') for s in ('random_ekf_03', 'random_ekf_09', 'random_ekf_21', 'other_ekf_H_dXi', 'edge_ekf_lam0')),
         tuple(('prefix_gh3', p) for p in ('lead9', 'chunk60_70', 'odd', 'mixed')),
         (('random_cubature_00', 'mixed'), ('random_cubature_03', 'odd')),
         (('random_gh3_08', 'mixed'),))


def case_name(source, pattern):
    return f'{source}.{pattern}'.replace('.', '__')


def gapped_case(Z, source, pattern):
    """The case of exact_grad_cases.npz with NaN over the pattern's ranges (clipped to the record), as make_exact_grad_cases._job takes it."""
    c = mf.load_case(Z, source)
    ys = np.array(c['ys'], dtype=np.float64)
    T = ys.size
    spans = tuple((max(a, 0), min(b, T)) for a, b in PATTERNS[pattern](T) if max(a, 0) < min(b, T))      # (a range past a short record: dropped)
    for a, b in spans:
        ys[a:b] = np.nan
    c.update(name=case_name(source, pattern), source=source, pattern=pattern, ys=ys, gaps=np.array(spans, dtype=np.int64).reshape(-1, 2))
    return c


def _job(args):
    """make_exact_grad_cases._job's pass with NaN measurements skipped and every observed step's innovation and its variance noted:
    -> (final NLL, [(nu_t, S_t)] over the observed steps, finite and PD)."""
    steps = []
    update = mg.linear_update

    def gapped(mp_, Pp, H, Xi, y):
        if mp.isnan(y):                                # the measurement alone decides
            return mp_, Pp, mpf(0)
        nu = y - sum(h * v for h, v in zip(H, mp_))
        S = sum(h * v for h, v in zip(H, mf.mx.matvec(Pp, H))) + Xi
        steps.append((nu, S))
        return update(mp_, Pp, H, Xi, y)
    mg.linear_update = gapped
    try:
        cum, ok = mg._job(args)
    finally:
        mg.linear_update = update
    return cum[-1], steps, ok


def evaluate(pool, cases, moved):
    """-> {name: (nll, grad [n_dir], F [n_dir][n_dir], n_observed, ok)}: value, central differences and the Fisher sum from the same passes."""
    jobs, keys = [], []
    for c in cases:
        nd = len(c['theta']) + (1 if c['with_dxi'] else 0)
        for k, sign in [(-1, 0)] + [(k, s) for k in range(nd) for s in (1, -1)]:
            if 0 <= k < len(c['theta']) and c['theta'][k] == -800.:
                continue
            jobs.append((c, k, sign, moved))
            keys.append((c['name'], k, sign))
    order = sorted(range(len(jobs)), key=lambda j: -len(jobs[j][0]['ys']) * mg.COST[jobs[j][0]['sigma']])      # longest passes first
    res = pool.map(_job, [jobs[j] for j in order], chunksize=1)
    vals = {keys[j]: r for j, r in zip(order, res)}
    out = {}
    for c in cases:
        nd = len(c['theta']) + (1 if c['with_dxi'] else 0)
        nll, base, ok = vals[(c['name'], -1, 0)]
        grad, up, dn = [], [], []
        for k in range(nd):
            if (c['name'], k, 1) not in vals:          # theta_lam = -800: a zero direction
                grad.append(mpf(0)); up.append(None); dn.append(None)
                continue
            (fu, su, ok1), (fd, sd, ok2) = vals[(c['name'], k, 1)], vals[(c['name'], k, -1)]
            assert len(su) == len(base) and len(sd) == len(base)
            grad.append((fu - fd) / (2 * mg.H_GRAD)); up.append(su); dn.append(sd)
            ok = ok and ok1 and ok2
        F = mf.fisher_prefixes(base, up, dn, (len(base),))[0]
        out[c['name']] = (nll, grad, F, len(base), ok)
    return out


def movements(e, m):
    """(value, relative; gradient, of its largest component; matrix, of its largest entry) between the exact and the moved evaluation."""
    gs = max(abs(v) for v in e[1])
    return (float(abs(m[0] - e[0]) / abs(e[0])), float(max(abs(a - b) for a, b in zip(e[1], m[1])) / gs), mf.movement(e[2], m[2]))


def main():
    procs = int(sys.argv[sys.argv.index('--procs') + 1]) if '--procs' in sys.argv else min(8, os.cpu_count() or 1)
    Z = np.load(os.path.join(OUT, 'exact_grad_cases.npz'))
    ZF = np.load(os.path.join(OUT, 'exact_fisher.npz'))
    cases = [gapped_case(Z, s, p) for line in CASES for s, p in line]
    with Pool(procs) as pool:
        exact, moved = evaluate(pool, cases, False), evaluate(pool, cases, True)
    out, kept, rejected, rejected_moved = {}, [], [], []
    for c in cases:
        n = c['name']
        e, m = exact[n], moved[n]
        ok = e[4] and m[4]
        dv, dg, dF = movements(e, m) if ok else (math.inf,) * 3
        good = ok and (c['exempt'] or (dv < mg.VALUE_MOVE_MAX and dg < mg.GRAD_MOVE_MAX and dF < mf.FISHER_MOVE_MAX))
        print(f"{n}: T {len(c['ys'])}, {e[3]} observed, {len(e[1])} directions, finite and PD {ok}, moved {dv:.2e} / {dg:.2e} / {dF:.2e} "
              f"-> {'admitted' if good else 'REJECTED'}", flush=True)
        if not good:
            rejected.append(n); rejected_moved.append((dv, dg, dF))
            continue
        kept.append(n)
        out.update({f'{n}.source': c['source'], f'{n}.pattern': c['pattern'], f'{n}.gaps': c['gaps'], f'{n}.ys': c['ys'], f'{n}.n_dir': len(e[1]),
                    f'{n}.n_observed': e[3], f'{n}.nll': float(e[0]), f'{n}.grad': np.array([float(v) for v in e[1]]),
                    f'{n}.fisher': np.array([[float(v) for v in r] for r in e[2]]), f'{n}.moved_nll': dv, f'{n}.moved_grad': dg, f'{n}.moved_fisher': dF})
    lines = [{case_name(s, p) for s, p in line} for line in CASES]
    if len(kept) < MIN_CASES or any(not line & set(kept) for line in lines):
        raise SystemExit(f'only {len(kept)} cases admitted ({rejected} rejected): a finding, not a reason to loosen the rule')
    # the pattern without a gap IS prefix_ekf: the stored value, gradient and matrix to the last digit
    none = case_name('prefix_ekf', 'none')
    assert out[f'{none}.nll'] == float(Z['prefix_ekf.nll']), (out[f'{none}.nll'], float(Z['prefix_ekf.nll']))
    assert np.array_equal(out[f'{none}.grad'], Z['prefix_ekf.grad']), (out[f'{none}.grad'], Z['prefix_ekf.grad'])
    assert np.array_equal(out[f'{none}.fisher'], ZF['prefix_ekf.fisher']), (out[f'{none}.fisher'], ZF['prefix_ekf.fisher'])
    out['names'] = np.array(sorted(kept))
    out['rejected'] = np.array(rejected, dtype='U48')
    out['rejected_moved'] = np.array(rejected_moved, dtype=np.float64).reshape(-1, 3)
    out['digits'] = mp.dps
    mg.save_npz(os.path.join(OUT, 'exact_gaps_grad.npz'), out)
    print(f'{len(kept)} cases admitted, {len(rejected)} rejected')


if __name__ == '__main__':
    main()
