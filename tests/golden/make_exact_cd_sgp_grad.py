"""Generates tests/golden/exact_cd_sgp_grad.npz: the continuous-discrete sigma-point MLE objective -- cd_sgp_filter(...)[-1][-1] of
build(g(theta)), filters_smoothers.py:534-582 with the right-hand side :124-137 and the RK4 step of quadratures.py:34-54 -- and its exact
gradient in 100-digit arithmetic.  tests/test_cd_sgp_gradient_host.py (a float64 restatement, no GPU) and
tests/test_gpu_cd_sgp_gradient.py (cgp_sgp_nll_grad on the SDE model) run against it.

The recursion is make_exact.py's (imported, not restated: build_chirp_model's drift and dispersion, cd_sgp_common, rk4, linear_update,
run_filter, the sigma-point sets); the case conventions -- records, admission, movement, entry names, the file's byte-stable writer -- are
make_exact_grad_cases.py's (imported as well), the draws follow make_exact_cd_grad.py's recipe (the same seeds and slots, 2 (sqrt(3) / ell) dt
<= 0.14, lam dt <= 0.004), narrowed at dt = 1e-2 to 2 pi g(v) dt <= 0.9 (random_case below says why).  The gradient is taken as there: central differences with a step of 1e-30 at 100
digits, at the float64 theta the tests pass to the kernel.  theta_lam = -800 stands for lam = 0 exactly.

A pass costs s points x 4 stages a step in Python arithmetic (7 ms a step with the cubature rule, 55 with Gauss-Hermite order 3, 170 with
order 4), so the records are shorter than the EKF fixtures': the lengths below are what keeps the whole file at some minutes on 8 cores.

Groups.
    prefix       one chirp record, every prefix 1 .. 130, once with the cubature rule and once with Gauss-Hermite order 3
                 (.nll_prefix, .grad_prefix)
    random_cds   16 seeded draws (random_case, records of 24 .. 48 steps): both builders, dt = 1e-3 and 1e-2, tracking and lost filters;
                 three of four with the cubature rule, every fourth with Gauss-Hermite order 3 (16 .. 24 steps)
    edge         theta_lam = -800 (lam = 0 exactly) and ell = 30; exempt from the conditioning rule, they carry their movement
    other        a non-unit H with d / d Xi as a seventh gradient entry (.with_dxi); Gauss-Hermite order 4 (256 points: the kernel's
                 re-evaluation path) on a record of 8 steps -- the RECORD is shortened for it, not the set
    gaps         six records with NaN samples, run as CGP_SKIP_MISSING runs them (a NaN sample: the RK4 prediction is the step's result and
                 the step adds nothing): at the first step, at the last step, in a run, scattered (Gauss-Hermite order 3), on the La Scala
                 builder at dt = 1e-2, and everywhere (value 0, gradient 0)
    substeps     n = 2 and n = 4 RK4 steps of dt / n between two measurements (.n)

Admission, as there: (a) finite with a positive-definite filtering covariance at every step, (b) value and gradient recomputed with every
measurement and every theta moved by 1e-15 of itself: the value moves by less than 1e-13 relative, the gradient by less than 1e-10 of its
largest component.  A rejected draw is replaced by the next seed of its slot (six draws a slot).  The file needs at least 12 admitted
draws, and at least three quarters of ALL draws admitted: if fewer are, narrow the draw (make_exact_cd_grad.py's region), not the gate.
Drawn / rejected / kept counts per group are stored.

Entries: make_exact_grad_cases.py's (method = 'cd_sgp_filter', sigma = 'cubature' | 'gh3' | 'gh4'), name.skip (1: the NaN samples are
gaps) and name.n (the substeps).

    python -m tests.golden.make_exact_cd_sgp_grad [--procs N]      (CPU only; 80 seconds on 8 cores: 10 CPU-minutes)
"""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

from tests.golden.make_exact import build_chirp_model, cd_sgp_common, chol, g, linear_update, rk4, run_filter
from tests.golden.make_exact_cd_grad import movement, with_nan
from tests.golden.make_exact_grad_cases import (GRAD_MOVE_MAX, H_GRAD, INIT, LASCALA_INIT, MOVE, VALUE_MOVE_MAX, case, g_inv64, save_npz,
                                                sigma_set, track_record)

OUT = os.path.dirname(os.path.abspath(__file__))
mp.dps = 100
SLOTS, MAX_DRAWS, MIN_KEPT = 16, 6, 12
LOST_BY = {1e-3: 25.0, 1e-2: 6.0}
V_MAX = {1e-3: 30.0, 1e-2: 8.0}
_SETS = {}


def _set(name):
    if name not in _SETS:
        _SETS[name] = sigma_set(name)
    return _SETS[name]


def nll_prefixes(sigma, params, Xi, dt, ys, H, skip, n):
    """cd_sgp_filter's cumulative NLL after every step (filters_smoothers.py:570-582), n RK4 steps of dt / n per measurement, and whether
    every filtering covariance had a Cholesky factor; H None = the builder's; skip: a NaN sample is a gap."""
    drift, disp, _, m0, P0, H0 = build_chirp_model(params)
    H = H0 if H is None else H
    sg = _set(sigma)
    h = dt / n

    def ode(m, P):
        return cd_sgp_common(sg, drift, disp, m, P)

    def step(mf, Pf, y):
        mp_, Pp = mf, Pf
        for _ in range(n):
            mp_, Pp = rk4(ode, mp_, Pp, h)
        if skip and mp.isnan(y):
            return mp_, Pp, mpf(0)
        return linear_update(mp_, Pp, H, Xi, y)
    rows = run_filter(step, m0, P0, ys)
    ok = all(mp.isfinite(r[2]) and mp.isfinite(chol(r[1])[0][0]) for r in rows)
    return [r[2] for r in rows], ok


def _job(args):
    """One filter pass of a case: k = -1 the value, 0 .. P - 1 theta_k +- h, P the measurement-noise variance Xi +- h; moved = the pass on
    the inputs moved by 1e-15 of themselves (make_exact_grad_cases.py: _job)."""
    c, k, sign, moved = args
    mp.dps = 100
    theta = [mpf(float(t)) for t in c['theta']]
    ys = [mpf(float(y)) for y in c['ys']]
    Xi, dt = mpf(float(c['Xi'])), mpf(float(c['dt']))
    P = len(theta)
    if moved:
        s = np.random.default_rng(7_000_000 + c['seed']).choice([-1, 1], size=P + len(ys))
        theta = [t * (1 + int(s[i]) * MOVE) for i, t in enumerate(theta)]
        ys = [y * (1 + int(s[P + i]) * MOVE) for i, y in enumerate(ys)]
    if 0 <= k < P:
        theta[k] += sign * H_GRAD
    elif k == P:
        Xi += sign * H_GRAD
    params = [mpf(0) if float(t0) == -800. else g(t) for t0, t in zip(c['theta'], theta)]       # theta = -800: lam = 0 exactly
    if c['build'] == 'lascala':
        params = [mpf(0), mpf(0)] + params
    H = None if c['H'] is None else [mpf(float(v)) for v in c['H']]
    try:
        cum, ok = nll_prefixes(c['sigma'], params, Xi, dt, ys, H, c['skip'], c['n'])
    except (ValueError, ZeroDivisionError):              # a covariance that lost its Cholesky factor inside an RK4 stage
        cum, ok = [mpf('nan')] * len(ys), False
    return (cum if c['prefix'] else cum[-1:]), ok


# ------------------------------------------------------------------------------------------------ the cases (NumPy only, seeded)
def cds_case(name, group, sigma, build, theta, ys, Xi, dt, seed, skip=False, n=1, **kw):
    c = case(name, group, 'cd_sgp_filter', sigma, build, theta, ys, Xi, dt, seed, **kw)
    c['skip'], c['n'] = bool(skip), int(n)
    return c


def random_case(i, draw):
    """Slot i, draw number `draw` (the next one when a draw is rejected): make_exact_cd_grad.py's recipe -- every fourth slot takes the La
    Scala builder; the slot fixes dt (1e-2 in two of three) and whether the filter starts lost (two of three) -- on 24 .. 48 steps (16 ..
    24 with Gauss-Hermite order 3, every fourth slot from slot 1), and NARROWED at dt = 1e-2: with that recipe's numbers there (track up to
    v = 12, a lost start 15 above it, sigma within a factor of 4) 9 of 25 draws were rejected, every one because the sigma-point moment
    ODE's covariance lost its Cholesky factor inside an RK4 step in the 100-digit run itself -- the spread of the rotation rate over the
    sigma points takes the explicit step out of its stability region, where the EKF's ODE, which sees the rate at the mean alone, stays
    inside.  So at dt = 1e-2 the track stays below v = 8, a lost filter starts 6 above it and sigma stays within a factor of 2; the gate is
    as it was."""
    seed = 40_000 + 100 * i + draw
    rng = np.random.default_rng(seed)
    lascala, gh3 = i % 4 == 3, i % 4 == 1
    lost, dt = i % 3 != 0, (1e-2 if i % 3 != 1 else 1e-3)
    T = int(rng.integers(16, 25) if gh3 else rng.integers(24, 49))
    Xi = 10 ** rng.uniform(-3, math.log10(3.0))
    vmax = V_MAX[dt]
    kind = rng.integers(0, 4)
    if kind == 0:
        v0, v1 = rng.uniform(-2, vmax, size=2)
    elif kind == 1:
        v0, v1 = rng.uniform(-2, 3.0, size=2)
    elif kind == 2:
        v0, v1 = rng.uniform(3.5, 7.0, size=2)
    else:
        v0 = rng.uniform(-2, vmax)
        v1 = float(np.clip(v0 + rng.uniform(-0.3, 0.3), -2, vmax))
    ys = track_record(rng, T, dt, Xi, v0, v1)
    spread = 4.0 ** rng.uniform(-1, 1, size=4 if lascala else 6)
    if dt == 1e-2:
        spread[-2] = math.sqrt(spread[-2])                               # sigma: within a factor of 2
    p = (LASCALA_INIT if lascala else INIT) * spread
    p[-1] = v0 + LOST_BY[dt] if lost else max(v0 + rng.uniform(-0.5, 0.5), 0.05)
    return cds_case(f'random_cds_{i:02d}', 'random_cds', 'gh3' if gh3 else 'cubature', 'lascala' if lascala else 'chirp', g_inv64(p), ys, Xi, dt, seed,
                    lost=lost)


def fixed_cases():
    out = []
    rng = np.random.default_rng(434343)
    ys130 = track_record(rng, 130, 1e-3, 0.1, 7.0, 9.0)
    ys130_l = track_record(rng, 130, 1e-2, 0.1, 6.5, 7.5)
    th, th_l = g_inv64(INIT), g_inv64(LASCALA_INIT)
    out.append(cds_case('prefix_cds_cubature', 'prefix', 'cubature', 'chirp', th, ys130, 0.1, 1e-3, 1, prefix=True))
    out.append(cds_case('prefix_cds_gh3', 'prefix', 'gh3', 'chirp', th, ys130, 0.1, 1e-3, 2, prefix=True))
    # ---- parameter edges on the first 40 steps of the chirp record
    ys40 = ys130[:40]
    t = th.copy()
    t[0] = -800.
    out.append(cds_case('edge_cds_lam0', 'edge', 'cubature', 'chirp', t, ys40, 0.1, 1e-3, 100, exempt=True))
    p = INIT.copy()
    p[3] = 30.
    out.append(cds_case('edge_cds_ell30', 'edge', 'cubature', 'chirp', g_inv64(p), ys40, 0.1, 1e-3, 101, exempt=True))
    # ---- a non-unit H (four random entries) with d / d Xi as a seventh gradient entry; the 256-point set
    H = np.random.default_rng(525252).uniform(-1.5, 1.5, size=4)
    out.append(cds_case('other_cds_H_dXi', 'other', 'cubature', 'chirp', th, ys40, 0.1, 1e-3, 4, H=H, with_dxi=True))
    out.append(cds_case('other_cds_gh4', 'other', 'gh4', 'chirp', th, ys130[:8], 0.1, 1e-3, 5))
    # ---- records with gaps
    scat = np.random.default_rng(535353).random(20) < 0.3
    out.append(cds_case('gaps_cds_first', 'gaps', 'cubature', 'chirp', th, with_nan(ys40, [0]), 0.1, 1e-3, 200, skip=True))
    out.append(cds_case('gaps_cds_last', 'gaps', 'cubature', 'chirp', th, with_nan(ys40, [39]), 0.1, 1e-3, 201, skip=True))
    out.append(cds_case('gaps_cds_run', 'gaps', 'cubature', 'chirp', th, with_nan(ys40, slice(5, 12)), 0.1, 1e-3, 202, skip=True))
    out.append(cds_case('gaps_cds_scattered', 'gaps', 'gh3', 'chirp', th, with_nan(ys130[:20], scat), 0.1, 1e-3, 203, skip=True))
    out.append(cds_case('gaps_cds_lascala_run', 'gaps', 'cubature', 'lascala', th_l, with_nan(ys130_l[:40], slice(14, 26)), 0.1, 1e-2, 204, skip=True))
    out.append(cds_case('gaps_cds_everywhere', 'gaps', 'cubature', 'chirp', th, np.full(12, np.nan), 0.1, 1e-3, 205, skip=True))
    # ---- substeps
    out.append(cds_case('substeps_cds_n2', 'substeps', 'cubature', 'chirp', th, ys130[:30], 0.1, 1e-3, 300, n=2))
    out.append(cds_case('substeps_cds_n4', 'substeps', 'cubature', 'lascala', th_l, ys130_l[:30], 0.1, 1e-2, 301, n=4))
    return out


# ------------------------------------------------------------------------------------------------ evaluation
def cost(job):
    c = job[0]
    return len(c['ys']) * c['n'] * {'cubature': 8, 'gh3': 81, 'gh4': 256}[c['sigma']]


def evaluate(pool, cases, moved):
    """Value and gradient (all prefixes for a prefix case) of every case: -> {name: (nll list, grad rows list, ok)}."""
    jobs, keys = [], []
    for c in cases:
        nd = len(c['theta']) + (1 if c['with_dxi'] else 0)
        for k, sign in [(-1, 0)] + [(k, s) for k in range(nd) for s in (1, -1)]:
            if 0 <= k < len(c['theta']) and c['theta'][k] == -800.:
                continue
            jobs.append((c, k, sign, moved))
            keys.append((c['name'], k, sign))
    order = sorted(range(len(jobs)), key=lambda j: -cost(jobs[j]))          # longest passes first
    res = pool.map(_job, [jobs[j] for j in order], chunksize=1)
    vals = {keys[j]: r for j, r in zip(order, res)}
    out = {}
    for c in cases:
        nd = len(c['theta']) + (1 if c['with_dxi'] else 0)
        base, ok = vals[(c['name'], -1, 0)]
        grad = []
        for k in range(nd):
            if (c['name'], k, 1) not in vals:
                grad.append([mpf(0)] * len(base))
                continue
            (up, ok1), (dn, ok2) = vals[(c['name'], k, 1)], vals[(c['name'], k, -1)]
            grad.append([(a - b) / (2 * H_GRAD) for a, b in zip(up, dn)])
            ok = ok and ok1 and ok2
        out[c['name']] = (base, grad, ok)
    return out


def main():
    procs = int(sys.argv[sys.argv.index('--procs') + 1]) if '--procs' in sys.argv else min(8, os.cpu_count() or 1)
    admitted, stats = [], {'random_cds': dict(drawn=SLOTS, rejected=0)}
    with Pool(procs) as pool:
        todo = fixed_cases()
        draw_of = {}
        for i in range(SLOTS):
            c = random_case(i, 0)
            draw_of[c['name']] = 0
            todo.append(c)
        while todo:
            exact, moved = evaluate(pool, todo, False), evaluate(pool, todo, True)
            again = []
            for c in todo:
                e, m = exact[c['name']], moved[c['name']]
                dv, dg = movement(e, m) if e[2] and m[2] else (math.inf, math.inf)
                good = e[2] and (c['exempt'] or (dv < VALUE_MOVE_MAX and dg < GRAD_MOVE_MAX))
                print(f"{c['name']} (seed {c['seed']}, {c['sigma']}): T {len(c['ys'])} finite and PD {e[2]}, moved {dv:.2e} / {dg:.2e} -> {'admitted' if good else 'REJECTED'}",
                      flush=True)
                if good:
                    admitted.append((c, e, dv, dg))
                elif c['group'] in stats:
                    stats[c['group']]['rejected'] += 1
                    d = draw_of[c['name']] + 1
                    if d >= MAX_DRAWS:
                        print(f"{c['name']}: {MAX_DRAWS} draws rejected -- the slot stays empty", flush=True)
                        continue
                    nc = random_case(int(c['name'][-2:]), d)
                    draw_of[nc['name']] = d
                    stats[c['group']]['drawn'] += 1
                    again.append(nc)
                else:
                    raise SystemExit(f"{c['name']}: a fixed case failed (finite and PD {e[2]}, moved {dv:.2e} / {dg:.2e})")
            todo = again
    kept = sum(a[0]['group'] == 'random_cds' for a in admitted)
    drawn = stats['random_cds']['drawn']
    if kept < MIN_KEPT or 4 * kept < 3 * drawn:
        raise SystemExit(f'random_cds: {kept} admitted of {drawn} drawn -- narrow its recipe, not the gate')
    admitted.sort(key=lambda a: a[0]['name'])
    out = {'names': np.array([a[0]['name'] for a in admitted]), 'digits': mp.dps}
    for c, (nll, grad, _), dv, dg in admitted:
        n = c['name']
        P = len(c['theta'])
        with np.errstate(over='ignore'):
            params = np.log(np.exp(c['theta']) + 1.)
        out.update({f'{n}.theta': c['theta'], f'{n}.params': params, f'{n}.ys': c['ys'], f'{n}.Xi': c['Xi'], f'{n}.dt': c['dt'],
                    f'{n}.H': np.array([0., 1., 0., 0.]) if c['H'] is None else c['H'], f'{n}.build': c['build'], f'{n}.method': c['method'],
                    f'{n}.sigma': c['sigma'], f'{n}.nll': float(nll[-1]), f'{n}.grad': np.array([float(r[-1]) for r in grad]),
                    f'{n}.group': c['group'], f'{n}.seed': c['seed'], f'{n}.lost': int(c['lost']), f'{n}.with_dxi': int(c['with_dxi']),
                    f'{n}.skip': int(c['skip']), f'{n}.n': c['n'], f'{n}.moved_nll': dv, f'{n}.moved_grad': dg})
        if c['prefix']:
            out[f'{n}.nll_prefix'] = np.array([float(v) for v in nll])
            out[f'{n}.grad_prefix'] = np.array([[float(v) for v in r] for r in grad]).T[:, :P]
    for grp, s in stats.items():
        out[f'drawn.{grp}'], out[f'rejected.{grp}'] = s['drawn'], s['rejected']
    for grp in sorted({a[0]['group'] for a in admitted}):
        out[f'count.{grp}'] = sum(a[0]['group'] == grp for a in admitted)
    save_npz(os.path.join(OUT, 'exact_cd_sgp_grad.npz'), out)
    print({k: int(v) for k, v in out.items() if k.startswith(('drawn', 'rejected', 'count'))})


if __name__ == '__main__':
    main()
