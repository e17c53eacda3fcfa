"""Generates tests/golden/exact_fisher.npz: the Fisher information of the filters' Gaussian innovations model,

    F[i][j] = sum over steps t of ( d nu_i d nu_j / S  +  d S_i d S_j / (2 S^2) ),    nu_t = y_t - H mp_t,   S_t = H Pp_t H^T + Xi,

in 100-digit arithmetic, for cases of tests/golden/exact_grad_cases.npz (read from that file by name: theta, ys, Xi, dt, H, build, method,
sigma).  tests/test_gpu_fisher.py runs cgp_ekf_nll_fisher and cgp_sgp_nll_fisher against it.

Nothing is restated: the recursion is make_exact.py's and the pass over a case -- the float64 inputs taken as exact, theta_k or Xi moved by
+-1e-30, the inputs moved by 1e-15 with seeded signs -- is make_exact_grad_cases._job.  That pass hands every step's predicted moments to
linear_update (filters_smoothers.py:55-68); here the call is wrapped to note nu_t and S_t, which the NLL is made of, on its way through.
d nu and d S are central differences with a step of 1e-30 along every theta_k, and along Xi where the case has with_dxi (its last
direction).  theta_lam = -800 stands for lam = 0 exactly: that direction is zero, and so are its row and column of F.

Cases: six random EKF cases, the T = 130 EKF record and its first 1, 7, 8 and 9 samples (the kernel's 8-step block and its tail), the
non-unit H with d / d Xi (7 directions), two parameter edges (lam = 0, ell = 30), three random Gauss-Hermite and two cubature cases, the
Gauss-Hermite non-unit H case, and the Gauss-Hermite sets of order 4 and 5 (625 points: the fan re-evaluated in every pass).

Admission, as make_exact_grad_cases: F is recomputed with every measurement and every theta moved by 1e-15 of itself and must move by less
than 1e-10 of its largest entry -- a hundredth of the gate the test applies (1e-8).  The edge_* cases are exempt and carry their
movement.  A case that fails is left out and listed, with its movement, under `rejected`; the file must keep at least 18 of the 22
cases and at least one of every line of CASES.

Entries: names; name.source (the case of exact_grad_cases.npz) / .T (its first T samples) / .n_dir / .fisher (n_dir, n_dir) / .moved_fisher;
rejected, rejected_moved.

    python -m tests.golden.make_exact_fisher [--procs N]      (CPU only; about six minutes on 8 cores)
"""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

import tests.golden.make_exact as mx
import tests.golden.make_exact_grad_cases as mg

OUT = os.path.dirname(os.path.abspath(__file__))
mp.dps = 100
FISHER_MOVE_MAX = 1e-10
PREFIX_T = (1, 7, 8, 9)
# one line of the list each: the fixture keeps at least one case of every line
CASES = (('random_ekf_00', 'random_ekf_03', 'random_ekf_06', 'random_ekf_09', 'random_ekf_14', 'random_ekf_21'),
         ('prefix_ekf',),
         ('other_ekf_H_dXi',),
         ('edge_ekf_lam0', 'edge_ekf_ell30'),
         ('random_gh3_00', 'random_gh3_03', 'random_gh3_08'),
         ('other_gh3_H_dXi',),
         ('random_cubature_00', 'random_cubature_03'),
         ('size_gh4', 'size_gh5'),
         tuple(f'prefix_ekf_T{n}' for n in PREFIX_T))
MIN_CASES = 18


def load_case(Z, name):
    """A case of exact_grad_cases.npz as the dict make_exact_grad_cases._job takes."""
    return dict(name=name, theta=Z[f'{name}.theta'], ys=Z[f'{name}.ys'], Xi=float(Z[f'{name}.Xi']), dt=float(Z[f'{name}.dt']),
                H=Z[f'{name}.H'], build=str(Z[f'{name}.build']), method=str(Z[f'{name}.method']), sigma=str(Z[f'{name}.sigma']),
                seed=int(Z[f'{name}.seed']), with_dxi=bool(int(Z[f'{name}.with_dxi'])), prefix=False,
                exempt=str(Z[f'{name}.group']) == 'edge')


def _job(args):
    """make_exact_grad_cases._job's pass with every step's innovation and its variance noted: -> ([(nu_t, S_t)], finite and PD)."""
    steps = []
    update = mg.linear_update

    def noting(mp_, Pp, H, Xi, y):
        nu = y - sum(h * v for h, v in zip(H, mp_))
        S = sum(h * v for h, v in zip(H, mx.matvec(Pp, H))) + Xi
        steps.append((nu, S))
        return update(mp_, Pp, H, Xi, y)
    mg.linear_update = noting
    try:
        _, ok = mg._job(args)
    finally:
        mg.linear_update = update
    return steps, ok


def fisher_prefixes(base, up, dn, lengths):
    """F over the first n steps for every n of `lengths` (ascending): base [(nu, S)], up / dn [direction][(nu, S)] at +- H_GRAD (None: a
    zero direction)."""
    nd = len(up)
    F = [[mpf(0)] * nd for _ in range(nd)]
    out, t0 = [], 0
    for n in lengths:
        for t in range(t0, n):
            S = base[t][1]
            dnu = [mpf(0) if up[k] is None else (up[k][t][0] - dn[k][t][0]) / (2 * mg.H_GRAD) for k in range(nd)]
            dS = [mpf(0) if up[k] is None else (up[k][t][1] - dn[k][t][1]) / (2 * mg.H_GRAD) for k in range(nd)]
            for i in range(nd):
                for j in range(nd):
                    F[i][j] += dnu[i] * dnu[j] / S + dS[i] * dS[j] / (2 * S * S)
        t0 = n
        out.append([list(r) for r in F])
    return out


def evaluate(pool, cases, moved):
    """-> {name: ({T: F}, ok)} with T the whole record and, for prefix_ekf, the lengths of PREFIX_T."""
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
        base, ok = vals[(c['name'], -1, 0)]
        up, dn = [], []
        for k in range(nd):
            if (c['name'], k, 1) not in vals:
                up.append(None); dn.append(None)
                continue
            (u, ok1), (d, ok2) = vals[(c['name'], k, 1)], vals[(c['name'], k, -1)]
            up.append(u); dn.append(d)
            ok = ok and ok1 and ok2
        T = len(c['ys'])
        lengths = (PREFIX_T if c['name'] == 'prefix_ekf' else ()) + (T,)
        out[c['name']] = (dict(zip(lengths, fisher_prefixes(base, up, dn, lengths))), ok)
    return out


def movement(Fa, Fb):
    """Largest movement of an entry over the largest entry."""
    scale = max(abs(v) for r in Fa for v in r)
    return float(max(abs(a - b) for ra, rb in zip(Fa, Fb) for a, b in zip(ra, rb)) / scale)


def main():
    procs = int(sys.argv[sys.argv.index('--procs') + 1]) if '--procs' in sys.argv else min(8, os.cpu_count() or 1)
    Z = np.load(os.path.join(OUT, 'exact_grad_cases.npz'))
    sources = [n for line in CASES[:-1] for n in line]
    cases = [load_case(Z, n) for n in sources]
    with Pool(procs) as pool:
        exact, moved = evaluate(pool, cases, False), evaluate(pool, cases, True)
    out, kept, rejected, rejected_moved = {}, [], [], []
    for c in cases:
        (Fe, ok_e), (Fm, ok_m) = exact[c['name']], moved[c['name']]
        for T in sorted(Fe):
            name = c['name'] if T == len(c['ys']) else f"{c['name']}_T{T}"
            dF = movement(Fe[T], Fm[T]) if ok_e and ok_m else math.inf
            good = ok_e and ok_m and (c['exempt'] or dF < FISHER_MOVE_MAX)
            print(f"{name}: T {T}, {len(Fe[T])} directions, finite and PD {ok_e and ok_m}, moved {dF:.2e} -> {'admitted' if good else 'REJECTED'}", flush=True)
            if not good:
                rejected.append(name); rejected_moved.append(dF)
                continue
            kept.append(name)
            out.update({f'{name}.source': c['name'], f'{name}.T': T, f'{name}.n_dir': len(Fe[T]),
                        f'{name}.fisher': np.array([[float(v) for v in r] for r in Fe[T]]), f'{name}.moved_fisher': dF})
    if len(kept) < MIN_CASES or any(not set(line) & set(kept) for line in CASES):
        raise SystemExit(f'only {len(kept)} cases admitted ({rejected} rejected): a finding, not a reason to loosen the rule')
    out['names'] = np.array(sorted(kept))
    out['rejected'] = np.array(rejected, dtype='U32')
    out['rejected_moved'] = np.array(rejected_moved, dtype=np.float64)
    out['digits'] = mp.dps
    mg.save_npz(os.path.join(OUT, 'exact_fisher.npz'), out)
    print(f'{len(kept)} cases admitted, {len(rejected)} rejected')


if __name__ == '__main__':
    main()
