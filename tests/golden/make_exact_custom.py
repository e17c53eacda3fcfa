"""Generates tests/golden/exact_custom_ops.npz and exact_custom_ring.npz: the two model families of tests/custom_exact.py -- what
tests/test_exact_custom.py and tests/test_gpu_custom_exact.py hand to cgp_model_from_source as device source -- evaluated in 100-digit
arithmetic, rounded to float64 at the end.  The recursion is make_exact.py's (imported, not restated: jacobian -- the complex step --,
linear_update, smoother_common, sgp_prediction, cd_sgp_common, rk4, run_filter, run_smoother, Cubature, GH3 and the list algebra).

exact_custom_ops.npz -- ONE step (T = 1) of ekf_for_kpt (filters_smoothers.py:298-311) per case, d = 3 and d = 8: F = I + 0.05 randn dense,
Sigma and P0 dense SPD, so Pp is dense and every component of grad h shows in mf, Pf and (through S) nll, a wrong value in the innovation.
A case is (operation, c, s, m0, y); the operation table is tests/custom_exact.py:OPS, one operation per overload of namespace cgp::ad.
Every operation has four generic points (mp = F m0 drawn with components of magnitude 0.3 .. 2.7, positive where the operation needs it;
pow: four per exponent 2, 3, 0.5, -1, 2.5, 1, 0) and its edge points:
    sin, cos, tanh at 0 and pow(0, e) for e = 0, 1, 2, 3         m0 = 0, so that mp = F m0 = 0 exactly in any arithmetic
    tanh at +-20 (1 - t^2 rounds to 0), softplus at -40, 30 and 700 (the naive form, still finite), log at 1 + 2^-30, exp at -700
                                                                 m0 = F^-1 target: mp[0] is the edge to a rounding, which is all they need
    c / D and D / D with a denominator of 1e-150, sqrt at 1e-200 operations of their own (div_cd_tiny, div_dd_tiny, sqrt_tiny): the tiny
        operand is u[0] * s INSIDE the model and the result is scaled back to O(1).  A state of 1e-150 itself would not do: mp = F m0 cannot
        be 1e-150 to a rounding with a dense F, the derivative 1e300 squares to infinity in S = H Pp H^T in float64 while the exact S is
        finite, and the oracle's complex step (1e-30) is larger than the point.
Not in the table: pow(0, 0.5) and sqrt(0).  Their derivative is infinite, so H, S and with them the whole update are NaN or infinite in
exact arithmetic too: there is no exact value to compare with.
A generic point at which the float64 NumPy evaluation (oracle/np_filters.py:ekf_for_kpt on the host callable) sits further than 16 x 2^-53
from the exact one, relative to an output array's largest entry, is redrawn; an edge point that does is an error to be redesigned.
The number of cases is not a multiple of 64 (a ragged last wavefront).

exact_custom_ring.npz -- the ring model (tests/custom_exact.py:RING) for d = 1 .. 8, T = 8, B = 2 records with different parameter rows and
measurements; dense H, non-zero m0, dense SPD P0, dense non-symmetric dispersion b.  All eight methods: ekf, eks, sgp_filter, sgp_smoother,
cd_ekf, cd_eks, cd_sgp_filter, cd_sgp_smoother with the cubature rule, and the four sigma-point ones with Gauss-Hermite order 3 at d = 2
('gh3.' keys).  The smoothers are fed the ROUNDED exact filtering rows, as tests/test_exact.py:test_smoothers_on_the_exact_filtering_rows.

    python -m tests.golden.make_exact_custom          (CPU only, under a minute; byte-identical on every run)
"""
import os
import sys

import numpy as np
from mpmath import mp, mpf

from tests.golden.make_exact import (GH3, Cubature, cd_sgp_common, cho_solve, jacobian, linear_update, madd, matmul, matvec, mscale, outer, rk4,
                                     run_filter, run_smoother, sgp_prediction, smoother_common, tr, vadd)
from tests import custom_exact as cx

OUT = os.path.dirname(os.path.abspath(__file__))
mp.dps = 100
EPS = 2.0 ** -53
REDRAW_AT = 16.0
POW_EXPONENTS = (2.0, 3.0, 0.5, -1.0, 2.5, 1.0, 0.0)


class MP:
    sin, cos, exp, log, sqrt, tanh = mp.sin, mp.cos, mp.exp, mp.log, mp.sqrt, mp.tanh

    @staticmethod
    def softplus(x):
        return mp.log(mp.exp(x) + 1)


def M_(A):
    return [[mpf(float(v)) for v in r] for r in np.atleast_2d(A)]


def V_(a):
    return [mpf(float(v)) for v in a]


def spd(rng, d, scale, floor):
    A = scale * rng.standard_normal((d, d))
    return A @ A.T + floor * np.eye(d)


def savez(name, **arrays):
    """np.savez_compressed without the time stamps: the same bytes on every run"""
    import io
    import zipfile
    path = os.path.join(OUT, name)
    with zipfile.ZipFile(path, 'w') as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(name, os.path.getsize(path), 'bytes', flush=True)


# ------------------------------------------------------------------------------------------------ the operation table
def kpt_step_exact(F, Sigma, P0, Xi, h, m0, y):
    """filters_smoothers.py:298-311 at 100 digits: (mf, Pf, nll) as float64"""
    Fm = M_(F)
    mp_ = matvec(Fm, V_(m0))
    Pp = madd(matmul(matmul(Fm, M_(P0)), tr(Fm)), M_(Sigma))
    Hk = jacobian(lambda x: [h(x)], mp_)[0]
    PH = matvec(Pp, Hk)
    Xi, y = mpf(float(Xi)), mpf(float(y))
    S = sum(a * v for a, v in zip(Hk, PH)) + Xi
    K = [v / S for v in PH]
    pred = h(mp_)
    nll = (mp.log(2 * mp.pi * S) + (y - pred) ** 2 / S) / 2
    mf, Pf = vadd(mp_, [k * (y - pred) for k in K]), madd(Pp, mscale(outer(K, K), S), -1)
    return np.array([float(v) for v in mf]), np.array([[float(v) for v in r] for r in Pf]), float(nll)


def distance(got, want):
    """max |float64 - exact| / max |exact| over each output array, units of 2^-53: tests/cases.py:max_rel_err"""
    worst = 0.0
    for g, w in zip(got, want):
        g, w = np.atleast_1d(g), np.atleast_1d(w)
        if not np.array_equal(np.isnan(g), np.isnan(w)) or np.any(np.isnan(w)):
            return np.inf
        worst = max(worst, float(np.max(np.abs(g - w)) / max(np.max(np.abs(w)), 1e-300) / EPS))
    return worst


def op_cases():
    """(label, operation, c, s, kind, target): kind 'generic' (target None: drawn), 'zero' (m0 = 0) or 'at' (mp[0] = target)"""
    out = []
    for name, _, _, _, _, _ in cx.OPS:
        if name == 'pow':
            for e in POW_EXPONENTS:
                out += [(f'pow^{e:g} #{k}', name, e, 0.0, 'generic', None) for k in range(4)]
            out += [(f'pow(0, {e:g})', name, e, 0.0, 'zero', None) for e in (0.0, 1.0, 2.0, 3.0)]
            continue
        c, s = 1.5, 0.0
        if name in ('div_cd_tiny', 'div_dd_tiny'):
            s = 1e-150
        if name == 'sqrt_tiny':
            c, s = 1e-100, 1e-200
        if name in ('deep', 'bump', 'logistic'):
            c = 0.7
        out += [(f'{name} #{k}', name, c, s, 'generic', None) for k in range(4)]
        if name in ('sin', 'cos', 'tanh'):
            out.append((f'{name}(0)', name, c, s, 'zero', None))
        for edge_of, t in (('tanh', 20.0), ('tanh', -20.0), ('softplus', -40.0), ('softplus', 30.0), ('softplus', 700.0), ('log', 1.0 + 2.0 ** -30),
                           ('exp', -700.0)):
            if name == edge_of:
                out.append((f'{name}({t:.10g})', name, c, s, 'at', t))
    return out


def main_ops():
    from oracle import np_filters as onf
    out = {'digits': mp.dps, 'op_names': np.array([op[0] for op in cx.OPS])}
    for d in (3, 8):
        rng = np.random.default_rng(100 + d)
        F = np.eye(d) + 0.05 * rng.standard_normal((d, d))
        Sigma, P0, Xi = spd(rng, d, 0.3, 0.05), spd(rng, d, 0.5, 0.2), 0.3
        rows, worst = [], {}
        for label, name, c, s, kind, target in op_cases():
            i = cx.OP_INDEX[name]
            positive = cx.OPS[i][2]
            q = np.array([float(i), c, s])
            for attempt in range(200):
                t = rng.uniform(0.3, 2.7, d) * (1.0 if positive else rng.choice([-1.0, 1.0], d))
                if kind == 'at':
                    t[0] = target
                m0 = np.zeros(d) if kind == 'zero' else np.linalg.solve(F, t)
                y = float(rng.standard_normal())
                u = F @ m0
                if kind == 'generic':
                    assert np.all(np.abs(u) > 0.29) and np.all(np.abs(u) < 2.71) and (not positive or np.all(u > 0)), (label, u)
                elif kind == 'at':
                    assert abs(u[0] - target) <= 4 * EPS * abs(target), (label, u[0])
                else:
                    assert not np.any(u), label
                exact = kpt_step_exact(F, Sigma, P0, Xi, cx.ops_host(q, d, MP), m0, y)
                got = onf.ekf_for_kpt(F, Sigma, cx.ops_host(q, d), Xi, m0, P0, 0.0, np.array([y]))
                a = distance((got[0][0], got[1][0], got[2][0]), exact)
                if a <= REDRAW_AT:
                    break
                assert kind == 'generic', f'{label} (d = {d}): the float64 evaluation is {a:.3g} x 2^-53 from exact -- redesign this edge point'
                print(f'  d = {d} {label}: {a:.3g} x 2^-53, redrawn', flush=True)
            else:
                raise AssertionError(f'{label}: no well-conditioned point in 200 draws')
            assert np.all(np.isfinite(exact[0])) and np.all(np.isfinite(exact[1])) and np.isfinite(exact[2]), label
            worst[name] = max(worst.get(name, 0.0), a)
            rows.append((label, q, m0, y) + exact)
        B = len(rows)
        assert B % 64 != 0, B
        print(f'd = {d}: {B} cases; float64 NumPy against exact, worst per operation (x 2^-53):', {k: round(v, 1) for k, v in worst.items()}, flush=True)
        pre = f'd{d}.'
        out.update({pre + 'F': F, pre + 'Sigma': Sigma, pre + 'P0': P0, pre + 'Xi': Xi, pre + 'label': np.array([r[0] for r in rows]),
                    pre + 'q': np.stack([r[1] for r in rows]), pre + 'op': np.array([int(r[1][0]) for r in rows]),
                    pre + 'm0': np.stack([r[2] for r in rows]), pre + 'y': np.array([r[3] for r in rows]),
                    pre + 'mf': np.stack([r[4] for r in rows]), pre + 'Pf': np.stack([r[5] for r in rows]), pre + 'nll': np.array([r[6] for r in rows])})
    savez('exact_custom_ops.npz', **out)


# ------------------------------------------------------------------------------------------------ the ring, d = 1 .. 8
def rows_f64(rows):
    """[(m, P[, nll])] of mpf -> float64 arrays (T, d), (T, d, d)[, (T,)]; the rounded P is symmetric to the bit"""
    out = [np.array([[float(v) for v in r[0]] for r in rows]), np.array([[[float(v) for v in row] for row in r[1]] for r in rows])]
    out[1] = np.tril(out[1]) + np.transpose(np.tril(out[1], -1), (0, 2, 1))
    if len(rows[0]) == 3:
        out.append(np.array([float(r[2]) for r in rows]))
    return out


def rounded(f):
    """the exact filtering rows as a float64 implementation receives them: rounded, then exact again"""
    m, P = rows_f64(f)[:2]
    return [(V_(m[k]), M_(P[k]), None) for k in range(m.shape[0])]


def ring_pipelines(p, b, H, Xi, m0, P0, dt, ys, sg, only_sigma):
    drift, cond = cx.ring_host(p, MP, lists=True)
    b, H, m0, P0, Xi, dt, ys = M_(b), V_(H), V_(m0), M_(P0), mpf(float(Xi)), mpf(float(dt)), V_(ys)
    gamma = matmul(b, tr(b))
    mean = lambda u: cond(u, dt)[0]
    res = {}

    def ekf_predict(mf, Pf):                                             # filters_smoothers.py:222-264
        J = jacobian(mean, mf)
        mp_, Sig = cond(mf, dt)
        return J, mp_, madd(matmul(matmul(J, Pf), tr(J)), Sig)

    def ekf_step(mf, Pf, y):
        _, mp_, Pp = ekf_predict(mf, Pf)
        return linear_update(mp_, Pp, H, Xi, y)

    def eks_step(ms, Ps, mf, Pf):                                       # :317-349
        J, mp_, Pp = ekf_predict(mf, Pf)
        return smoother_common(matmul(J, Pf), mf, Pf, mp_, Pp, ms, Ps)

    def sgpf_step(mf, Pf, y):                                           # :446-490
        mp_, Pp, _, _ = sgp_prediction(sg, cond, dt, mf, Pf)
        return linear_update(mp_, Pp, H, Xi, y)

    def sgps_step(ms, Ps, mf, Pf):                                      # :493-531
        mp_, Pp, chi, fm = sgp_prediction(sg, cond, dt, mf, Pf)
        D = madd(sg.expect_outer(chi, fm), outer(mf, mp_), -1)
        return smoother_common(tr(D), mf, Pf, mp_, Pp, ms, Ps)

    def cde_ode(m, P):                                                  # :384-385
        J = jacobian(drift, m)
        return drift(m), madd(madd(matmul(P, tr(J)), matmul(J, P)), gamma)

    def cde_step(mf, Pf, y):
        mp_, Pp = rk4(cde_ode, mf, Pf, dt)
        return linear_update(mp_, Pp, H, Xi, y)

    def cdes_ode(m, P, mf, Pf):                                         # :427-432
        A = madd(jacobian(drift, m), tr(cho_solve(Pf, tr(gamma))))
        sol = cho_solve(Pf, [[v] for v in vadd(m, mf, -1)])
        return vadd(drift(m), matvec(gamma, [r[0] for r in sol])), madd(madd(matmul(A, P), matmul(P, tr(A))), gamma, -1)

    def cdf_step(mf, Pf, y):                                            # :534-582
        mp_, Pp = rk4(lambda m, P: cd_sgp_common(sg, drift, b, m, P), mf, Pf, dt)
        return linear_update(mp_, Pp, H, Xi, y)

    def cds_ode(m, P, mf, Pf):                                          # :585-632
        G = cho_solve(Pf, gamma)
        _m, _P = cd_sgp_common(sg, drift, b, m, P)
        return vadd(_m, matvec(tr(G), vadd(m, mf, -1))), madd(madd(madd(_P, matmul(tr(G), P)), matmul(P, G)), mscale(gamma, 2), -1)

    pairs = [('sgp_filter', 'sgp_smoother', sgpf_step, sgps_step), ('cd_sgp_filter', 'cd_sgp_smoother', cdf_step, lambda ms, Ps, mf, Pf: rk4(cds_ode, ms, Ps, -dt, mf, Pf))]
    if not only_sigma:
        pairs += [('ekf', 'eks', ekf_step, eks_step), ('cd_ekf', 'cd_eks', cde_step, lambda ms, Ps, mf, Pf: rk4(cdes_ode, ms, Ps, -dt, mf, Pf))]
    for fname, sname, fstep, sstep in pairs:
        f = run_filter(fstep, m0, P0, ys)
        res[fname], res[sname] = rows_f64(f), rows_f64(run_smoother(sstep, rounded(f)))
    return res


def ring_inputs(d):
    """float64 inputs of dimension d, drawn with NumPy only"""
    rng = np.random.default_rng(200 + d)
    B, T = 2, 8
    p = np.array([0.8, 0.6, 0.3, 0.05, 0.4]) * rng.uniform(0.8, 1.25, (B, 5))
    b = 0.3 * np.eye(d) + 0.15 * rng.standard_normal((d, d))
    H = rng.uniform(0.4, 1.0, d) * rng.choice([-1.0, 1.0], d)
    m0 = 0.6 * rng.standard_normal(d)
    return dict(p=p, b=b, H=H, Xi=0.3, m0=m0, P0=spd(rng, d, 0.3, 0.2), dt=0.05, ys=rng.standard_normal((B, T)))


def main_ring():
    out = {'digits': mp.dps}
    for d in range(1, 9):
        z = ring_inputs(d)
        out.update({f'd{d}.in.{k}': v for k, v in z.items()})
        for pre, sg, only_sigma in ((f'd{d}.', Cubature(d), False),) + ((('gh3.', GH3(2), True),) if d == 2 else ()):
            per = [ring_pipelines(z['p'][i], z['b'], z['H'], z['Xi'], z['m0'], z['P0'], z['dt'], z['ys'][i], sg, only_sigma) for i in range(2)]
            for fn in per[0]:
                for k in range(len(per[0][fn])):
                    out[f'{pre}{fn}.{k}'] = np.stack([r[fn][k] for r in per])
            print(pre, 'done', flush=True)
    savez('exact_custom_ring.npz', **out)


if __name__ == '__main__':
    if '--ring' not in sys.argv:
        main_ops()
    if '--ops' not in sys.argv:
        main_ring()
