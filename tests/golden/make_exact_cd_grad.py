"""Generates tests/golden/exact_cd_grad.npz: the continuous-discrete MLE objective -- cd_ekf(...)[-1][-1] of build(g(theta)),
filters_smoothers.py:352-397 with the RK4 step of quadratures.py:34-54 -- and its exact gradient in 100-digit arithmetic.
tests/test_cd_gradient_host.py (a float64 restatement, no GPU) and tests/test_gpu_cd_gradient.py (cgp_cd_ekf_nll_grad) run against it.

The recursion is make_exact.py's (imported, not restated: build_chirp_model's drift and dispersion, jacobian, rk4, linear_update,
run_filter); the case conventions -- records, admission, movement, entry names, the file's byte-stable writer -- are
make_exact_grad_cases.py's (imported as well).  The gradient is taken as there: central differences with a step of 1e-30 at 100 digits,
at the float64 theta the tests pass to the kernel.  theta_lam = -800 stands for lam = 0 exactly.

Groups.
    prefix       one chirp and one La Scala record, every prefix 1 .. 130 (.nll_prefix, .grad_prefix)
    random_cd    16 seeded draws: both builders, dt = 1e-3 and 1e-2, tracking and lost filters
    edge         theta_lam = -800 (lam = 0 exactly) and ell = 30; exempt from the conditioning rule, they carry their movement
    other        a non-unit H with d / d Xi as a seventh gradient entry (.with_dxi)
    gaps         six records with NaN samples, run as CGP_SKIP_MISSING runs them (a NaN sample: the RK4 prediction is the step's result and
                 the step adds nothing): at the first step, at the last step, in a run across a measurement block of eight, scattered,
                 on the La Scala builder at dt = 1e-2, and everywhere (value 0, gradient 0)
The draws keep RK4 inside its stability region, or the reference itself diverges: 2 (sqrt(3) / ell) dt <= 0.14 and lam dt <= 0.004 (ell and
lam within a factor of 4 of the demos' start point), and the rotation 2 pi g(v) dt <= 1.7 (at dt = 1e-2 the track stays below v = 12 and a
lost filter starts 15 above it, where make_exact_grad_cases.py's discrete cases go to 25 and start 25 above).

Admission, as there: (a) finite with a positive-definite filtering covariance at every step, (b) value and gradient recomputed with every
measurement and every theta moved by 1e-15 of itself: the value moves by less than 1e-13 relative, the gradient by less than 1e-10 of its
largest component.  A rejected draw is replaced by the next seed of its slot (six draws a slot); the file needs at least 5 of every 6
slots of the random group and every fixed case.  Drawn / rejected / kept counts per group are stored.

Entries: make_exact_grad_cases.py's (method = 'cd_ekf', sigma = ''), and name.skip (1: the NaN samples are gaps).

    python -m tests.golden.make_exact_cd_grad [--procs N]      (CPU only; 48 seconds on 8 cores: 6 CPU-minutes)
"""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

from tests.golden.make_exact import build_chirp_model, chol, g, jacobian, linear_update, madd, matmul, rk4, run_filter, tr
from tests.golden.make_exact_grad_cases import (GRAD_MOVE_MAX, H_GRAD, INIT, LASCALA_INIT, MOVE, VALUE_MOVE_MAX, case, g_inv64, save_npz,
                                                track_record)

OUT = os.path.dirname(os.path.abspath(__file__))
mp.dps = 100
SLOTS, MAX_DRAWS = 16, 6
LOST_BY = {1e-3: 25.0, 1e-2: 15.0}
V_MAX = {1e-3: 30.0, 1e-2: 12.0}


def nll_prefixes(params, Xi, dt, ys, H, skip):
    """cd_ekf's cumulative NLL after every step (filters_smoothers.py:384-397) and whether every filtering covariance had a Cholesky
    factor; H None = the builder's; skip: a NaN sample is a gap."""
    drift, disp, _, m0, P0, H0 = build_chirp_model(params)
    H = H0 if H is None else H
    gamma = matmul(disp, tr(disp))

    def ode(m, P):                                                       # :384-385
        J = jacobian(drift, m)
        return drift(m), madd(madd(matmul(P, tr(J)), matmul(J, P)), gamma)

    def step(mf, Pf, y):
        mp_, Pp = rk4(ode, mf, Pf, dt)
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
    cum, ok = nll_prefixes(params, Xi, dt, ys, H, c['skip'])
    return (cum if c['prefix'] else cum[-1:]), ok


# ------------------------------------------------------------------------------------------------ the cases (NumPy only, seeded)
def cd_case(name, group, build, theta, ys, Xi, dt, seed, skip=False, **kw):
    c = case(name, group, 'cd_ekf', '', build, theta, ys, Xi, dt, seed, **kw)
    c['skip'] = bool(skip)
    return c


def random_case(i, draw):
    """Slot i, draw number `draw` (the next one when a draw is rejected), as make_exact_grad_cases.py's random_case: every fourth slot takes
    the La Scala builder; the slot fixes dt (1e-2 in two of three) and whether the filter starts lost (two of three)."""
    seed = 40_000 + 100 * i + draw
    rng = np.random.default_rng(seed)
    lascala = i % 4 == 3
    lost, dt = i % 3 != 0, (1e-2 if i % 3 != 1 else 1e-3)
    T = int(rng.integers(40, 131))
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
    p = (LASCALA_INIT if lascala else INIT) * 4.0 ** rng.uniform(-1, 1, size=4 if lascala else 6)
    p[-1] = v0 + LOST_BY[dt] if lost else max(v0 + rng.uniform(-0.5, 0.5), 0.05)
    return cd_case(f'random_cd_{i:02d}', 'random_cd', 'lascala' if lascala else 'chirp', g_inv64(p), ys, Xi, dt, seed, lost=lost)


def with_nan(ys, where):
    out = np.array(ys, dtype=np.float64)
    out[where] = np.nan
    return out


def fixed_cases():
    out = []
    rng = np.random.default_rng(434343)
    ys130 = track_record(rng, 130, 1e-3, 0.1, 7.0, 9.0)
    ys130_l = track_record(rng, 130, 1e-2, 0.1, 6.5, 7.5)
    th, th_l = g_inv64(INIT), g_inv64(LASCALA_INIT)
    out.append(cd_case('prefix_cd_chirp', 'prefix', 'chirp', th, ys130, 0.1, 1e-3, 1, prefix=True))
    out.append(cd_case('prefix_cd_lascala', 'prefix', 'lascala', th_l, ys130_l, 0.1, 1e-2, 2, prefix=True))
    # ---- parameter edges on the first 80 steps of the chirp record
    t = th.copy()
    t[0] = -800.
    out.append(cd_case('edge_cd_lam0', 'edge', 'chirp', t, ys130[:80], 0.1, 1e-3, 100, exempt=True))
    p = INIT.copy()
    p[3] = 30.
    out.append(cd_case('edge_cd_ell30', 'edge', 'chirp', g_inv64(p), ys130[:80], 0.1, 1e-3, 101, exempt=True))
    # ---- a non-unit H (four random entries) with d / d Xi as a seventh gradient entry
    H = np.random.default_rng(525252).uniform(-1.5, 1.5, size=4)
    out.append(cd_case('other_cd_H_dXi', 'other', 'chirp', th, ys130[:80], 0.1, 1e-3, 4, H=H, with_dxi=True))
    # ---- records with gaps
    ys80, scat = ys130[:80], np.random.default_rng(535353).random(80) < 0.3
    out.append(cd_case('gaps_cd_first', 'gaps', 'chirp', th, with_nan(ys80, [0]), 0.1, 1e-3, 200, skip=True))
    out.append(cd_case('gaps_cd_last', 'gaps', 'chirp', th, with_nan(ys80, [79]), 0.1, 1e-3, 201, skip=True))
    out.append(cd_case('gaps_cd_run', 'gaps', 'chirp', th, with_nan(ys80, slice(5, 12)), 0.1, 1e-3, 202, skip=True))      # steps 5 .. 11: across 7 | 8
    out.append(cd_case('gaps_cd_scattered', 'gaps', 'chirp', th, with_nan(ys80, scat), 0.1, 1e-3, 203, skip=True))
    out.append(cd_case('gaps_cd_lascala_run', 'gaps', 'lascala', th_l, with_nan(ys130_l[:80], slice(14, 26)), 0.1, 1e-2, 204, skip=True))
    out.append(cd_case('gaps_cd_everywhere', 'gaps', 'chirp', th, np.full(20, np.nan), 0.1, 1e-3, 205, skip=True))
    return out


# ------------------------------------------------------------------------------------------------ evaluation
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
    order = sorted(range(len(jobs)), key=lambda j: -len(jobs[j][0]['ys']))      # longest passes first
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


def movement(a, b):
    """make_exact_grad_cases.py's movement; a value or a gradient that is exactly zero (a record of NaN only) moves by its absolute change."""
    (na, ga, _), (nb, gb, _) = a, b
    vs = abs(na[-1]) if na[-1] != 0 else mpf(1)
    scale = max(abs(r[-1]) for r in ga)
    scale = scale if scale != 0 else mpf(1)
    return float(abs(nb[-1] - na[-1]) / vs), float(max(abs(x[-1] - y[-1]) for x, y in zip(ga, gb)) / scale)


def main():
    procs = int(sys.argv[sys.argv.index('--procs') + 1]) if '--procs' in sys.argv else min(8, os.cpu_count() or 1)
    admitted, stats = [], {'random_cd': dict(drawn=SLOTS, rejected=0)}
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
                print(f"{c['name']} (seed {c['seed']}): T {len(c['ys'])} finite and PD {e[2]}, moved {dv:.2e} / {dg:.2e} -> {'admitted' if good else 'REJECTED'}", flush=True)
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
    kept = sum(a[0]['group'] == 'random_cd' for a in admitted)
    if 6 * kept < 5 * SLOTS:
        raise SystemExit(f'random_cd: {kept} of {SLOTS} slots filled -- narrow its recipe')
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
                    f'{n}.skip': int(c['skip']), f'{n}.moved_nll': dv, f'{n}.moved_grad': dg})
        if c['prefix']:
            out[f'{n}.nll_prefix'] = np.array([float(v) for v in nll])
            out[f'{n}.grad_prefix'] = np.array([[float(v) for v in r] for r in grad]).T[:, :P]
    for grp, s in stats.items():
        out[f'drawn.{grp}'], out[f'rejected.{grp}'] = s['drawn'], s['rejected']
    for grp in sorted({a[0]['group'] for a in admitted}):
        out[f'count.{grp}'] = sum(a[0]['group'] == grp for a in admitted)
    save_npz(os.path.join(OUT, 'exact_cd_grad.npz'), out)
    print({k: int(v) for k, v in out.items() if k.startswith(('drawn', 'rejected', 'count'))})


if __name__ == '__main__':
    main()
