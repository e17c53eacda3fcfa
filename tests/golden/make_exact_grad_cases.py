"""Generates tests/golden/exact_grad_cases.npz: the MLE objective -- ekf(...)[-1][-1] and sgp_filter(...)[-1][-1] of build(g(theta)) -- and
its exact gradient in 100-digit arithmetic AT THE EDGES: every record length 1 .. 130 of one record per method, seeded random parameter
vectors and records (tracking and "lost" filters, dt = 1e-3 and 1e-2, both builders), the parameter region where the model constants'
formulas cancel (lam -> 0, large ell), Gauss-Hermite orders 4 and 5, a non-unit H and the derivative with respect to Xi.
tests/test_gpu_gradient_edges.py runs cgp_ekf_nll_grad and cgp_sgp_nll_grad against it.

The recursion is make_exact.py's (imported, not restated: build_chirp_model, jacobian, sgp_prediction, linear_update, run_filter, GH3,
Cubature); the gradient is taken as there, by central differences with a step of 1e-30 at 100 digits, at the float64 theta the tests
pass to the kernels.  Added here: the Gauss-Hermite rule of any order (GH), a measurement row H other than the builder's, the cumulative
NLL of every prefix of a record (the filter's own running sum), and the derivative with respect to Xi (a seventh gradient entry).
theta_lam = -800 stands for lam = 0 exactly (float64 g(-800) is 0: the builder's other branch); its gradient entry, 1e-348 in size, is 0.

Admission.  A drawn case enters the file only if (a) the 100-digit run stays finite with a positive-definite filtering covariance at every
step and (b) the recursion is well conditioned there: value and gradient are recomputed with every measurement and every theta moved by
1e-15 of itself (random signs); the value must move by less than 1e-13 relative and the gradient by less than 1e-10 of its largest
component -- a hundredth of the gates the tests apply (1e-11, 1e-8).  A rejected draw is replaced by the next seed of its slot; seeds,
draws and rejections per group are stored.  The named parameter-edge cases are exempt from (b) -- their conditioning is the finding --
and every case carries its movement (name.moved_nll, name.moved_grad).

Entries: name.theta / .params / .ys / .Xi / .dt / .H / .build / .method / .sigma / .nll / .grad (/ .nll_prefix, .grad_prefix for the
prefix cases; .grad has a seventh entry, d / d Xi, where name.with_dxi is 1), .group, .seed, .lost, .moved_nll, .moved_grad; names,
drawn.<group>, rejected.<group>, count.<group>.

    python -m tests.golden.make_exact_grad_cases [--procs N]      (CPU only; 4.5 minutes on 8 cores: 36 CPU-minutes)
"""
import functools
import math
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

import tests.golden.make_exact as mx
from tests.golden.make_exact import GH3, Cubature, build_chirp_model, g, jacobian, linear_update, run_filter, sgp_prediction, madd, matmul, tr, chol

OUT = os.path.dirname(os.path.abspath(__file__))
mp.dps = 100
H_GRAD = mpf(10) ** -30
MOVE = mpf(10) ** -15
VALUE_MOVE_MAX, GRAD_MOVE_MAX = 1e-13, 1e-10
INIT = np.array([0.1, 0.1, 0.1, 1., 1., 7.])                        # demos/ekfs_mle.py: lam, b, delta, ell, sigma, m0_v
LASCALA_INIT = np.array([0.1, 1., 1., 7.])                          # delta, ell, sigma, m0_v
LOST_BY = 25.0
mx.m32_solution = functools.lru_cache(maxsize=64)(mx.m32_solution)   # state-independent: once per parameter vector, not once per sigma point


class GH(GH3):
    """SigmaPoints.gauss_hermite(d, order), quadratures.py:156-196, for any order: the roots of the probabilists' Hermite polynomial He_n
    (He_{k+1} = x He_k - k He_{k-1}), weights n! / (n He_{n-1}(x))^2 (they sum to 1); dimension 0 varies fastest."""
    def __init__(self, d, order):
        polys = [[mpf(1)], [mpf(1), mpf(0)]]                        # coefficients, highest power first
        for k in range(1, order):
            a, b = polys[k] + [mpf(0)], [mpf(0), mpf(0)] + [k * c for c in polys[k - 1]]
            polys.append([x - y for x, y in zip(a, b)])
        nodes = [mp.re(r) for r in mp.polyroots(polys[order], maxsteps=500, extraprec=1000)]
        w1 = [mp.factorial(order) / (order * mp.polyval(polys[order - 1], x)) ** 2 for x in nodes]
        self.xi, self.w = [], []
        for n in range(order ** d):
            idx = [(n // order ** r) % order for r in range(d)]
            self.xi.append([nodes[i] for i in idx])
            wt = mpf(1)
            for i in idx:
                wt *= w1[i]
            self.w.append(wt)


def sigma_set(name):
    return {'gh3': lambda: GH3(4), 'cubature': lambda: Cubature(4), 'gh4': lambda: GH(4, 4), 'gh5': lambda: GH(4, 5)}[name]()


def nll_prefixes(method, sigma, params, Xi, dt, ys, H):
    """The filter's cumulative NLL after every step (filters_smoothers.py:222-264 / 446-490) and whether every filtering covariance had a
    Cholesky factor; H None = the builder's."""
    _, _, cond, m0, P0, H0 = build_chirp_model(params)
    H = H0 if H is None else H
    if method == 'ekf':
        def step(mf, Pf, y):
            J = jacobian(lambda u: cond(u, dt)[0], mf)
            mp_, Sig = cond(mf, dt)
            return linear_update(mp_, madd(matmul(matmul(J, Pf), tr(J)), Sig), H, Xi, y)
    else:
        sg = sigma_set(sigma)

        def step(mf, Pf, y):
            mp_, Pp, _, _ = sgp_prediction(sg, cond, dt, mf, Pf)
            return linear_update(mp_, Pp, H, Xi, y)
    rows = run_filter(step, m0, P0, ys)
    ok = all(mp.isfinite(r[2]) and mp.isfinite(chol(r[1])[0][0]) for r in rows)
    return [r[2] for r in rows], ok


def _job(args):
    """One filter pass of a case: k = -1 the value, 0 .. P - 1 theta_k +- h, P the measurement-noise variance Xi +- h; moved = the pass on
    the inputs moved by 1e-15 of themselves."""
    case, k, sign, moved = args
    mp.dps = 100
    theta = [mpf(float(t)) for t in case['theta']]
    ys = [mpf(float(y)) for y in case['ys']]
    Xi, dt = mpf(float(case['Xi'])), mpf(float(case['dt']))
    P = len(theta)
    if moved:
        s = np.random.default_rng(7_000_000 + case['seed']).choice([-1, 1], size=P + len(ys))
        theta = [t * (1 + int(s[i]) * MOVE) for i, t in enumerate(theta)]
        ys = [y * (1 + int(s[P + i]) * MOVE) for i, y in enumerate(ys)]
    if 0 <= k < P:
        theta[k] += sign * H_GRAD
    elif k == P:
        Xi += sign * H_GRAD
    params = [mpf(0) if float(t0) == -800. else g(t) for t0, t in zip(case['theta'], theta)]       # theta = -800: lam = 0 exactly
    if case['build'] == 'lascala':
        params = [mpf(0), mpf(0)] + params
    H = None if case['H'] is None else [mpf(float(v)) for v in case['H']]
    cum, ok = nll_prefixes(case['method'], case['sigma'], params, Xi, dt, ys, H)
    return (cum if case['prefix'] else cum[-1:]), ok


# ------------------------------------------------------------------------------------------------ the cases (NumPy only, seeded)
def g_inv64(p):
    return np.log(np.expm1(np.asarray(p, dtype=np.float64)))


def _softplus(v):
    return np.logaddexp(0.0, v)


def track_record(rng, T, dt, Xi, v0, v1):
    """tests/test_gpu_fuzz.py: make_set -- a raised-cosine frequency-state track from v0 towards v1, random amplitude and phase."""
    cyc = rng.uniform(0.3, 2.5)
    v = v0 + (v1 - v0) * 0.5 * (1 - np.cos(2 * math.pi * cyc * np.arange(T) / T))
    phase = np.cumsum(_softplus(v)) * dt
    amp = rng.uniform(0.5, 2.0)
    return amp * np.sin(2 * math.pi * phase + rng.uniform(0, 2 * math.pi)) + math.sqrt(Xi) * rng.standard_normal(T)


def case(name, group, method, sigma, build, theta, ys, Xi, dt, seed, H=None, prefix=False, with_dxi=False, lost=False, exempt=False):
    return dict(name=name, group=group, method=method, sigma=sigma, build=build, theta=np.asarray(theta, dtype=np.float64),
                ys=np.asarray(ys, dtype=np.float64), Xi=float(Xi), dt=float(dt), seed=int(seed), H=None if H is None else np.asarray(H, dtype=np.float64),
                prefix=prefix, with_dxi=with_dxi, lost=bool(lost), exempt=exempt)


def random_case(group, method, sigma, i, draw):
    """Slot i of a random group, draw number `draw` (0 first; the next one when a draw is rejected).  Every fourth slot takes the La Scala
    builder; the slot fixes dt (1e-2 in two of three) and whether the filter starts LOST_BY away from the track (two of three), so that the
    admitted set holds both whatever is rejected."""
    seed = {'ekf': 10_000, 'gh3': 20_000, 'cubature': 30_000}[sigma or 'ekf'] + 100 * i + draw
    rng = np.random.default_rng(seed)
    lascala = i % 4 == 3
    lost, dt = i % 3 != 0, (1e-2 if i % 3 != 1 else 1e-3)
    T = int(rng.integers(40, 131))
    Xi = 10 ** rng.uniform(-3, math.log10(3.0))
    vmax = 30.0 if dt == 1e-3 else 25.0
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
    p[-1] = v0 + LOST_BY if lost else max(v0 + rng.uniform(-0.5, 0.5), 0.05)
    return case(f'random_{sigma or "ekf"}_{i:02d}', group, method, sigma, 'lascala' if lascala else 'chirp', g_inv64(p), ys, Xi, dt, seed, lost=lost)


# The frequency state below -30: m0_v = g(theta) is positive, so the state has to be DRIVEN there.  A loose frequency prior (a large sigma)
# on a constant record does it within a few steps; LOW_SEED was searched with the float64 port for a final state below -30 (and a finite NLL).
LOW_PARAMS = np.array([0.1, 0.1, 0.1, 1.0, 30., 0.05])              # (the port's EKF ends at -56 on this record)
LOW_XI, LOW_T, LOW_AMP, LOW_SEED = 0.01, 80, 1.0, 2


def low_record():
    rng = np.random.default_rng(616161 + LOW_SEED)
    return LOW_AMP + math.sqrt(LOW_XI) * rng.standard_normal(LOW_T)


def fixed_cases():
    out = []
    rng = np.random.default_rng(424242)
    ys130 = track_record(rng, 130, 1e-3, 0.1, 7.0, 9.0)
    th = g_inv64(INIT)
    for method, sigma in (('ekf', ''), ('sgp_filter', 'gh3'), ('sgp_filter', 'cubature')):
        out.append(case(f'prefix_{sigma or "ekf"}', 'prefix', method, sigma, 'chirp', th, ys130, 0.1, 1e-3, 1, prefix=True))
    # ---- parameter edges, EKF and GH-3 each, on the first 80 steps of that record (high / low: records of their own)
    edges = [('lam0', 0, None), ('lam1e-3', 0, 1e-3), ('lam1e-6', 0, 1e-6), ('lam1e-9', 0, 1e-9), ('ell30', 3, 30.), ('ell0.02', 3, 0.02), ('b1e-4', 1, 1e-4), ('sigma10', 4, 10.)]
    ys_high = track_record(np.random.default_rng(424243), 80, 1e-3, 0.1, 38.0, 39.5)
    ys_low = low_record()
    for method, sigma in (('ekf', ''), ('sgp_filter', 'gh3')):
        tag = sigma or 'ekf'
        for n, (label, k, v) in enumerate(edges):
            p = INIT.copy()
            if v is not None:
                p[k] = v
            t = g_inv64(p)
            if v is None:
                t[k] = -800.
            out.append(case(f'edge_{tag}_{label}', 'edge', method, sigma, 'chirp', t, ys130[:80], 0.1, 1e-3, 100 + n, exempt=True))
        p = INIT.copy()
        p[5] = 38.0
        out.append(case(f'edge_{tag}_freq_high', 'edge', method, sigma, 'chirp', g_inv64(p), ys_high, 0.1, 1e-3, 120, exempt=True))
        out.append(case(f'edge_{tag}_freq_low', 'edge', method, sigma, 'chirp', g_inv64(LOW_PARAMS), ys_low, LOW_XI, 1e-3, 121, exempt=True))
    # ---- sigma-set sizes: Gauss-Hermite orders 4 (256 points) and 5 (625) on one record
    out.append(case('size_gh4', 'size', 'sgp_filter', 'gh4', 'chirp', th, ys130[:64], 0.1, 1e-3, 2))
    out.append(case('size_gh5', 'size', 'sgp_filter', 'gh5', 'chirp', th, ys130[:40], 0.1, 1e-3, 3))
    # ---- a non-unit H (four random entries) with d / d Xi as a seventh gradient entry
    H = np.random.default_rng(515151).uniform(-1.5, 1.5, size=4)
    for method, sigma in (('ekf', ''), ('sgp_filter', 'gh3')):
        out.append(case(f'other_{sigma or "ekf"}_H_dXi', 'other', method, sigma, 'chirp', th, ys130[:80], 0.1, 1e-3, 4, H=H, with_dxi=True))
    return out


GROUPS = (('random_ekf', 'ekf', '', 24), ('random_gh3', 'sgp_filter', 'gh3', 10), ('random_cubature', 'sgp_filter', 'cubature', 6))
MAX_DRAWS = 6
COST = {'': 1, 'cubature': 2, 'gh3': 12, 'gh4': 40, 'gh5': 100}


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
    order = sorted(range(len(jobs)), key=lambda j: -len(jobs[j][0]['ys']) * COST[jobs[j][0]['sigma']])     # longest passes first
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
    """Relative movement of the final value; movement of the final gradient over its largest component."""
    (na, ga, _), (nb, gb, _) = a, b
    scale = max(abs(r[-1]) for r in ga)
    return float(abs(nb[-1] - na[-1]) / abs(na[-1])), float(max(abs(x[-1] - y[-1]) for x, y in zip(ga, gb)) / scale)


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name, v in arrays.items():
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w') as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def main():
    procs = int(sys.argv[sys.argv.index('--procs') + 1]) if '--procs' in sys.argv else min(8, os.cpu_count() or 1)
    admitted, stats = [], {}
    with Pool(procs) as pool:
        todo = fixed_cases()
        draw_of = {}
        for grp, method, sigma, n in GROUPS:
            stats[grp] = dict(drawn=n, rejected=0)
            for i in range(n):
                c = random_case(grp, method, sigma, i, 0)
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
                        raise SystemExit(f"{c['name']}: {MAX_DRAWS} draws rejected -- narrow the recipe of {c['group']}")
                    grp, method, sigma, _ = next(g_ for g_ in GROUPS if g_[0] == c['group'])
                    nc = random_case(grp, method, sigma, int(c['name'][-2:]), d)
                    draw_of[nc['name']] = d
                    stats[grp]['drawn'] += 1
                    again.append(nc)
                else:
                    raise SystemExit(f"{c['name']}: a fixed case failed (finite and PD {e[2]}, moved {dv:.2e} / {dg:.2e})")
            todo = again
    for grp, s in stats.items():
        if 2 * s['rejected'] > s['drawn']:
            raise SystemExit(f'{grp}: {s["rejected"]} of {s["drawn"]} draws rejected -- narrow its recipe')
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
                    f'{n}.moved_nll': dv, f'{n}.moved_grad': dg})
        if c['prefix']:
            out[f'{n}.nll_prefix'] = np.array([float(v) for v in nll])
            out[f'{n}.grad_prefix'] = np.array([[float(v) for v in r] for r in grad]).T[:, :P]
    for grp, s in stats.items():
        out[f'drawn.{grp}'], out[f'rejected.{grp}'] = s['drawn'], s['rejected']
    for grp in sorted({a[0]['group'] for a in admitted}):
        out[f'count.{grp}'] = sum(a[0]['group'] == grp for a in admitted)
    save_npz(os.path.join(OUT, 'exact_grad_cases.npz'), out)
    print({k: int(v) for k, v in out.items() if k.startswith(('drawn', 'rejected', 'count'))})


if __name__ == '__main__':
    main()
