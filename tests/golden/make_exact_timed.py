"""Generates tests/golden/exact_timed.npz: the four continuous-discrete methods with one interval per step (`dts=`,
include/chirpgp_hip_timed.h) in 100-digit arithmetic, rounded to float64 at the end.

    python -m tests.golden.make_exact_timed          (about twenty seconds)

Nothing of the path is restated that tests/golden/make_exact.py states: the RK4 step, the scans, the sigma-point moment ODE, the update, the
model and the complex-step Jacobian are ITS `rk4`, `run_filter`, `run_smoother`, `cd_sgp_common`, `linear_update`, `build_chirp_model` and
`jacobian`, imported; the two moment ODEs of cd_ekf / cd_eks are the three lines they are in its `pipelines_rest` (filters_smoothers.py:384-385,
427-432).  What is new is the definition of the timed call, and it is driven step by step so that it cannot hide in a scan:
    filter, step t:          run_filter(step(dts[t]), m, P, [ys[t]])                      -- dts[0] from (m0, P0) to sample 0
    smoother, step t+1 -> t: run_smoother(step(dts[t + 1]), [row t of the filter, (ms, Ps)])  -- dts[0] never read
    a NaN sample (gap):      the prediction is the step's result, its NLL increment 0
    substeps n:              the refined record -- NaN at the inserted times -- over dts[t] / n repeated n times, rows n - 1, 2 n - 1, ... kept
Cases, on the chirp and the La Scala builders (the latter: build_chirp_model at lam = b = 0, as make_exact.py's main_lascala), the record of
tests/cases.py:chirp_case, dt = 1e-3, Gauss-Hermite order 3:
    jitter   T = 32   dts = dt (1 + 0.75 u), u = default_rng(5).uniform(-1, 1, T)
    zero3x   T = 32   the same with dts[12] = 3 dt and dts[20] = 0 (two samples at one instant)
    sub3     T = 16   the jittered grid with n = 3 substeps
    gaps     T = 32   the jittered grid, samples 0, 5 .. 8, 20 and 31 missing
The file holds float64 arrays only; a case's name is the prefix of its keys."""
import os
import sys

import numpy as np

from tests.golden.make_exact import (mp, mpf, rk4, run_filter, run_smoother, cd_sgp_common, linear_update, build_chirp_model, jacobian, cho_solve,
                                      matmul, matvec, madd, vadd, mscale, tr, GH3, to_f64, ROOT, OUT)

DT = 1e-3
BUILDERS = {'chirp': [0.1, 0.1, 0.1, 1., 1., 7.], 'lascala': [0., 0., 0.1, 1., 1., 7.]}      # lam, b, delta, ell, sigma, m0_v


def grids_and_records():
    """(case, n, dts, ys): float64 inputs, drawn with NumPy only"""
    sys.path.insert(0, ROOT)
    from tests import cases
    ys = cases.chirp_case(T=32).ys
    jitter = DT * (1.0 + 0.75 * np.random.default_rng(5).uniform(-1.0, 1.0, 32))
    special = jitter.copy()
    special[12], special[20] = 3 * DT, 0.0
    gapped = ys.copy()
    gapped[[0, 5, 6, 7, 8, 20, 31]] = np.nan
    return (('jitter', 1, jitter, ys), ('zero3x', 1, special, ys), ('sub3', 3, jitter[:16].copy(), ys[:16].copy()), ('gaps', 1, jitter, gapped))


def timed_filter(predict, H, Xi, m0, P0, dts, ys):
    """predict(m, P, dt) -> (mp, Pp).  One call of make_exact's run_filter per step, on that step's sample with that step's interval."""
    def step_of(dt):
        def step(mf, Pf, y):
            mp_, Pp = predict(mf, Pf, dt)
            if mp.isnan(y):                                             # a gap: the measurement alone decides
                return mp_, Pp, mpf(0)
            return linear_update(mp_, Pp, H, Xi, y)
        return step
    m, P, nll, rows = m0, P0, mpf(0), []
    for dt, y in zip(dts, ys):
        m, P, inc = run_filter(step_of(dt), m, P, [y])[0]
        nll += inc
        rows.append((m, P, nll))
    return rows


def timed_smoother(back, filt, dts):
    """back(ms, Ps, mf, Pf, dt): one backward step over dt.  One call of make_exact's run_smoother per step, over dts[t + 1]."""
    rows = [(filt[-1][0], filt[-1][1])]
    for t in range(len(filt) - 2, -1, -1):
        dt = dts[t + 1]
        rows.append(run_smoother(lambda ms, Ps, mf, Pf: back(ms, Ps, mf, Pf, dt), [filt[t], rows[-1] + (None,)])[0])
    return rows[::-1]


def methods(params, Xi):
    drift, b, _, m0, P0, H = build_chirp_model(params)
    gamma = matmul(b, tr(b))
    sg = GH3()

    def cde_ode(m, P):                                                  # filters_smoothers.py:384-385
        J = jacobian(drift, m)
        return drift(m), madd(madd(matmul(P, tr(J)), matmul(J, P)), gamma)

    def cdeks_ode(m, P, mf, Pf):                                        # :427-432
        A = madd(jacobian(drift, m), tr(cho_solve(Pf, tr(gamma))))
        sol = cho_solve(Pf, [[v] for v in vadd(m, mf, -1)])
        return vadd(drift(m), matvec(gamma, [r[0] for r in sol])), madd(madd(matmul(A, P), matmul(P, tr(A))), gamma, -1)

    def cdsgps_ode(m, P, mf, Pf):                                       # :615-621
        G = cho_solve(Pf, gamma)
        _m, _P = cd_sgp_common(sg, drift, b, m, P)
        return vadd(_m, matvec(tr(G), vadd(m, mf, -1))), madd(madd(madd(_P, matmul(tr(G), P)), matmul(P, G)), mscale(gamma, 2), -1)
    pairs = {
        'cd_ekf': (lambda m, P, dt: rk4(cde_ode, m, P, dt), lambda ms, Ps, mf, Pf, dt: rk4(cdeks_ode, ms, Ps, -dt, mf, Pf)),
        'cd_sgp_filter': (lambda m, P, dt: rk4(lambda m_, P_: cd_sgp_common(sg, drift, b, m_, P_), m, P, dt),
                          lambda ms, Ps, mf, Pf, dt: rk4(cdsgps_ode, ms, Ps, -dt, mf, Pf)),
    }
    return pairs, H, mpf(float(Xi)), m0, P0


def main():
    Xi = 0.1
    out = {'digits': float(mp.dps), 'Xi': Xi, 'dt': DT}
    for build, params in BUILDERS.items():
        pairs, H, Xi_, m0, P0 = methods(params, Xi)
        out[f'{build}.params'] = np.array(params)
        for case, n, dts, ys in grids_and_records():
            name = f'{build}_{case}'
            print(name, flush=True)
            out.update({f'{name}.dts': dts, f'{name}.ys': ys, f'{name}.n': float(n)})
            fine = [mpf(float(v) / n) for v in dts for _ in range(n)]      # h_t = dts[t] / n, ONE float64 division as the header defines it, n times
            ref = [mpf('nan')] * (n * len(ys))
            ref[n - 1::n] = [mpf(float(y)) for y in ys]                  # (float('nan') -> mpf nan)
            res = {}
            for (filt, smoo), (predict, back) in zip((('cd_ekf', 'cd_eks'), ('cd_sgp_filter', 'cd_sgp_smoother')), (pairs['cd_ekf'], pairs['cd_sgp_filter'])):
                f = timed_filter(predict, H, Xi_, m0, P0, fine, ref)
                s = timed_smoother(back, f, fine)
                res[filt], res[smoo] = f[n - 1::n], s[n - 1::n]
            out.update({f'{name}.{k}': v for k, v in to_f64(res).items()})
    np.savez_compressed(os.path.join(OUT, 'exact_timed.npz'), **out)


if __name__ == '__main__':
    main()
