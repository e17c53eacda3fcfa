"""Run-time compiled models (csrc/cgp_custom.hpp) against 100-digit arithmetic, the CPU half: the NumPy oracle on host callables of the two
model families of tests/custom_exact.py against tests/golden/exact_custom_ops.npz / exact_custom_ring.npz (tests/golden/make_exact_custom.py).
Its measured distance (pytest -s) DEFINES the gates the HIP kernels are held to in tests/test_gpu_custom_exact.py: about a decade above
the oracle's worst figure of the group, as in tests/test_exact.py -- never a figure the kernels produced."""
import os
import re

import numpy as np
import pytest

from tests import cases as cs
from tests import custom_exact as cx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = 2.0 ** -53
# max |float64 - exact| / max |exact| per output array of one case, units of 2^-53, NumPy oracle, worst case of the group over d = 3 and 8
# (pytest -s): arith 9.7 (mul_cd #0, d = 3), func 4.8 (sin #0, d = 3), pow 5.2 (pow^2 #2, d = 8), comp 7.2 (deep #0, d = 3).  Gates: about a decade above.
GATE_OPS = {'arith': 100., 'func': 50., 'pow': 50., 'comp': 100.}
# every committed case of the table is this well conditioned (the generator redraws a generic point that is not)
CONDITION = 16.
# the ring, worst over d = 1 .. 8, both records and the Gauss-Hermite run at d = 2, NumPy oracle (pytest -s): ekf 22 (d = 7), eks 30 (d = 2),
# sgp_filter 37 (d = 8), sgp_smoother 69 (d = 2), cd_ekf 11 (d = 7), cd_eks 3.3 (d = 5), cd_sgp_filter 11 (d = 8), cd_sgp_smoother 3.5 (d = 3).
# Gates: about a decade above.
GATE_RING = {'ekf': 200., 'eks': 300., 'sgp_filter': 400., 'sgp_smoother': 700., 'cd_ekf': 100., 'cd_eks': 40., 'cd_sgp_filter': 100., 'cd_sgp_smoother': 40.}


def load(name):
    return np.load(os.path.join(GOLD, name + '.npz'))


def distance(got, want):
    """the worst of cs.max_rel_err over the output arrays, units of 2^-53; NaN positions must be identical (asserted there)"""
    return max(cs.max_rel_err(g, w) / EPS for g, w in zip(got, want))


def check_ops(z, d, got, who):
    """Every case of the table against its exact value under its group's gate -- none skipped, none masked: (worst per operation, its label)"""
    worst = {}
    B = z[f'd{d}.op'].size
    assert got[0].shape == (B, d) and got[1].shape == (B, d, d) and got[2].shape == (B,)
    failed = []
    for b in range(B):
        name, group = cx.OPS[z[f'd{d}.op'][b]][:2]
        label = str(z[f'd{d}.label'][b])
        try:
            each = [distance((got[k][b],), (z[f'd{d}.{n}'][b],)) for k, n in enumerate(('mf', 'Pf', 'nll'))]
        except AssertionError:
            each = [np.inf] * 3                                            # NaN where the exact value is finite
        a = max(each)
        if a > worst.get(name, (-1., ''))[0]:
            worst[name] = (a, f"{label}, in {('mf', 'Pf', 'nll')[int(np.argmax(each))]}")
        if not a < GATE_OPS[group]:
            failed.append((label, a))
    for name, (a, label) in worst.items():
        print(f'ops d = {d} {who:5s} {name:12s} {a:8.3g} x 2^-53  ({label})')
    for group in cx.GROUPS:
        a, label = max(v for k, v in worst.items() if cx.OPS[cx.OP_INDEX[k]][1] == group)
        print(f'ops d = {d} {who:5s} group {group:6s} {a:8.3g} x 2^-53  ({label}), gate {GATE_OPS[group]:g}')
    assert not failed, (who, d, failed)
    return worst


@pytest.mark.parametrize('d', [3, 8])
def test_numpy_oracle_on_the_operation_table(d):
    from oracle import np_filters as onf
    z = load('exact_custom_ops')
    assert int(z['digits']) >= 40 and tuple(z['op_names']) == tuple(op[0] for op in cx.OPS)
    B = z[f'd{d}.op'].size
    assert B % 64 != 0 and set(z[f'd{d}.op']) == set(range(len(cx.OPS)))
    F, Sigma, P0, Xi = z[f'd{d}.F'], z[f'd{d}.Sigma'], z[f'd{d}.P0'], float(z[f'd{d}.Xi'])
    rows = [onf.ekf_for_kpt(F, Sigma, cx.ops_host(z[f'd{d}.q'][b], d), Xi, z[f'd{d}.m0'][b], P0, 0.0, z[f'd{d}.y'][b:b + 1]) for b in range(B)]
    got = tuple(np.stack([r[k][0] for r in rows]) for k in range(3))
    worst = check_ops(z, d, got, 'numpy')
    assert max(a for a, _ in worst.values()) <= CONDITION, worst


def ring_inputs(z, d):
    return {k: z[f'd{d}.in.{k}'] for k in ('p', 'b', 'H', 'Xi', 'm0', 'P0', 'dt', 'ys')}


def ring_sets(d):
    """(fixture key prefix, sigma-point set, methods): cubature for all eight, Gauss-Hermite order 3 for the sigma-point four at d = 2"""
    from chirpgp_amd.quadratures import SigmaPoints
    return ((f'd{d}.', SigmaPoints.cubature(d), cx.METHODS),) + ((('gh3.', SigmaPoints.gauss_hermite(2, 3), cx.SIGMA_METHODS),) if d == 2 else ())


def check_ring(z, d, pre, methods, got, who):
    out = {}
    for fn in methods:
        n = 3 if fn in cx.METHODS[::2] else 2
        a = max(distance([got[fn][k][i] for k in range(n)], [z[f'{pre}{fn}.{k}'][i] for k in range(n)]) for i in range(2))
        print(f'ring {pre:4s} {who:5s} {fn:16s} {a:8.3g} x 2^-53, gate {GATE_RING[fn]:g}')
        out[fn] = a
    bad = {fn: a for fn, a in out.items() if not a < GATE_RING[fn]}
    assert not bad, (who, pre, bad)
    return out


@pytest.mark.parametrize('d', range(1, 9))
def test_numpy_oracle_on_the_ring(d):
    """all eight methods on host callables of the ring; the smoothers on the rounded exact filtering rows"""
    from oracle import np_filters as onf
    z = load('exact_custom_ring')
    i_ = ring_inputs(z, d)
    H, Xi, m0, P0, dt, b = i_['H'], float(i_['Xi']), i_['m0'], i_['P0'], float(i_['dt']), i_['b']
    for pre, sg, methods in ring_sets(d):
        osg = cs.osig(sg)
        got = {fn: [] for fn in methods}
        for i in range(2):
            drift, cond = cx.ring_host(i_['p'][i])
            ys = i_['ys'][i]
            rows = lambda fn: (z[f'{pre}{fn}.0'][i], z[f'{pre}{fn}.1'][i])
            run = {'ekf': lambda: onf.ekf(cond, H, Xi, m0, P0, dt, ys), 'eks': lambda: onf.eks(cond, *rows('ekf'), dt),
                   'sgp_filter': lambda: onf.sgp_filter(cond, osg, H, Xi, m0, P0, dt, ys), 'sgp_smoother': lambda: onf.sgp_smoother(cond, osg, *rows('sgp_filter'), dt),
                   'cd_ekf': lambda: onf.cd_ekf(drift, lambda _: b, H, Xi, m0, P0, dt, ys), 'cd_eks': lambda: onf.cd_eks(drift, lambda _: b, *rows('cd_ekf'), dt),
                   'cd_sgp_filter': lambda: onf.cd_sgp_filter(drift, b, osg, H, Xi, m0, P0, dt, ys),
                   'cd_sgp_smoother': lambda: onf.cd_sgp_smoother(drift, b, osg, *rows('cd_sgp_filter'), dt)}
            for fn in methods:
                got[fn].append(run[fn]())
        got = {fn: [np.stack([r[k] for r in v]) for k in range(len(v[0]))] for fn, v in got.items()}
        check_ring(z, d, pre, methods, got, 'numpy')


def declared_in_namespace_ad():
    """The functions and operators csrc/cgp_custom.hpp defines in namespace ad, as 'name(argument types)': plain text matching on declarations"""
    text = open(os.path.join(ROOT, 'chirpgp_amd', 'csrc', 'cgp_custom.hpp')).read()
    body = text[text.index('namespace ad {'):text.index('}  // namespace ad')]
    found = set()
    for line in body.splitlines():
        m = re.match(r'\s*(?:template <int N> )?CGP_DEV (?:Dual<N>&?|double) (operator\S+?|\w+)\(([^)]*)\)', line)
        if m:
            kinds = ['Dual' if 'Dual<N>' in a else a.split()[-2] if len(a.split()) > 1 else a for a in m.group(2).split(',')]
            found.add(f'{m.group(1)}({",".join(kinds)})')
        elif re.match(r'\s*__device__ Dual\(double \w+\)', line):
            found.add('Dual(double)')
    return found


def test_every_overload_of_namespace_ad_is_an_operation_of_the_table():
    """A future overload cannot arrive untested: it has to be named by an operation of tests/custom_exact.py:OPS."""
    declared = declared_in_namespace_ad()
    assert len(declared) >= 29 and {'operator/(Dual,Dual)', 'operator-(Dual)', 'operator*=(Dual,double)', 'pow(Dual,double)', 'softplus(double)',
                                    'Dual(double)', 'chain(Dual,double,double)'} <= declared, sorted(declared)
    named = {sig for op in cx.OPS for sig in op[5]}
    assert declared <= named, f'no operation of the table runs {sorted(declared - named)}'
    assert named <= declared, f'the table names declarations the header does not have: {sorted(named - declared)}'
