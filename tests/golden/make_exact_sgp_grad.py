"""Generates tests/golden/exact_sgp_grad.npz: the sigma-point filter's MLE objective -- sgp_filter(build(g(theta)), ...)[-1][-1], the
objective of demos/ghfs_mle.py:53-56 and the La Scala GHFS job -- and its exact gradient, in 100-digit arithmetic.

The recursion is make_exact.py's (imported, not restated): SigmaPoints.gauss_hermite(4, 3) / cubature(4), sgp_prediction
(filters_smoothers.py:88-121), linear_update (:55-68), build_chirp_model (the La Scala model is its lam = b = 0 case, make_exact.py:
main_lascala).  The gradient is taken as exact_gradient does for the EKF: central differences with a step of 1e-30 at 100 digits
(truncation 1e-60 relative), at the float64 theta the tests pass to the kernel.

Entries (name.theta / .nll / .grad / .ys / .Xi / .dt / .build / .sigma):
    gh3_track, gh3_lost       the two records of exact_grad.npz (their ys, theta, Xi, dt), Gauss-Hermite order 3, chirp builder
    cubature_track            the first record with the cubature rule
    lascala_gh3_track         the first record, La Scala builder (delta, ell, sigma, m0_v = 0.1, 1, 1, 7), Gauss-Hermite order 3

    python -m tests.golden.make_exact_sgp_grad        (48 filter passes in a process pool: some minutes)
"""
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

from tests.golden.make_exact import GH3, Cubature, build_chirp_model, g, linear_update, sgp_prediction

OUT = os.path.dirname(os.path.abspath(__file__))
mp.dps = 100
H_GRAD = mpf(10) ** -30


def sgp_final_nll(params, Xi, dt, ys, sg):
    """sgp_filter(...)[2][-1] for mpf parameters lam, b, delta, ell, sigma, m0_v."""
    _, _, cond, m0, P0, H = build_chirp_model(params)
    Sig = cond([mpf(0)] * 4, dt)[1]                   # state-independent: evaluated once instead of at each of the s points

    def cond_fast(u, dt_):                            # the builder's cond_m_cov with its constants hoisted (same formulas)
        return cond_mean(u), Sig
    lam, ell, sigma = params[0], params[3], params[4]
    e = mp.exp(-lam * dt)
    gam = mp.sqrt(3) / ell
    eta = dt * gam
    ee = mp.exp(-eta)
    Fm = [[(1 + eta) * ee, dt * ee], [-dt * gam ** 2 * ee, (1 - eta) * ee]]

    def cond_mean(u):
        w = 2 * mp.pi * g(u[2])
        c, s = mp.cos(dt * w), mp.sin(dt * w)
        return [e * (c * u[0] - s * u[1]), e * (s * u[0] + c * u[1]), Fm[0][0] * u[2] + Fm[0][1] * u[3], Fm[1][0] * u[2] + Fm[1][1] * u[3]]
    mf, Pf, nll = m0, P0, mpf(0)
    for y in ys:
        mp_, Pp, _, _ = sgp_prediction(sg, cond_fast, dt, mf, Pf)
        mf, Pf, inc = linear_update(mp_, Pp, H, Xi, y)
        nll += inc
    return nll


def _params(build, theta):
    p = [g(t) for t in theta]
    return p if build == 'chirp' else [mpf(0), mpf(0)] + p


def _job(args):
    build, sigma, theta, Xi, dt, ys, k, sign = args
    mp.dps = 100
    theta = [mpf(float(t)) for t in theta]
    if k >= 0:
        theta[k] += sign * H_GRAD
    sg = GH3(4) if sigma == 'gh3' else Cubature(4)
    return sgp_final_nll(_params(build, theta), mpf(float(Xi)), mpf(float(dt)), [mpf(float(y)) for y in ys], sg)


def entries():
    z = np.load(os.path.join(OUT, 'exact_grad.npz'))
    rec = {n: (z[f'{n}.theta'], float(z[f'{n}.Xi']), float(z[f'{n}.dt']), z[f'{n}.ys']) for n in ('exact_track', 'exact_lost')}
    la_p = np.array([0.1, 1., 1., 7.])
    la_theta = np.log(np.expm1(la_p))                 # g_inv in float64: the kernel is evaluated at exactly this theta
    t, Xi, dt, ys = rec['exact_track']
    return [('gh3_track', 'chirp', 'gh3') + rec['exact_track'],
            ('gh3_lost', 'chirp', 'gh3') + rec['exact_lost'],
            ('cubature_track', 'chirp', 'cubature') + rec['exact_track'],
            ('lascala_gh3_track', 'lascala', 'gh3', la_theta, Xi, dt, ys)]


def main():
    ents = entries()
    jobs, keys = [], []
    for name, build, sigma, theta, Xi, dt, ys in ents:
        for k, sign in [(-1, 0)] + [(k, s) for k in range(len(theta)) for s in (1, -1)]:
            jobs.append((build, sigma, theta, Xi, dt, ys, k, sign))
            keys.append((name, k, sign))
    procs = int(sys.argv[sys.argv.index('--procs') + 1]) if '--procs' in sys.argv else os.cpu_count()
    with Pool(procs) as pool:
        vals = dict(zip(keys, pool.map(_job, jobs, chunksize=1)))
    out = {}
    for name, build, sigma, theta, Xi, dt, ys in ents:
        grad = np.array([float((vals[(name, k, 1)] - vals[(name, k, -1)]) / (2 * H_GRAD)) for k in range(len(theta))])
        out.update({f'{name}.theta': np.asarray(theta, dtype=np.float64), f'{name}.nll': float(vals[(name, -1, 0)]), f'{name}.grad': grad,
                    f'{name}.ys': np.asarray(ys, dtype=np.float64), f'{name}.Xi': Xi, f'{name}.dt': dt,
                    f'{name}.build': build, f'{name}.sigma': sigma})
        print(name, out[f'{name}.nll'], grad, flush=True)
    np.savez_compressed(os.path.join(OUT, 'exact_sgp_grad.npz'), digits=mp.dps, **out)


if __name__ == '__main__':
    main()
