"""The timed methods (`dts=`) against 100-digit arithmetic: tests/golden/exact_timed.npz, written by tests/golden/make_exact_timed.py from
tests/golden/make_exact.py's own RK4 step, scans, moment ODE and update, driven step by step -- it shares no code with oracle/ and none with
tests/times_oracle.py, so it pins the stepped NumPy oracle itself: the meaning of dts[0], the zero and the 3 dt interval, substeps, gaps.

Cases (both builders): a jittered grid, one with a zero and a 3 dt interval, n = 3 substeps, gaps.  Gates: those of tests/test_exact.py for
the same methods, max |float64 - exact| / max |exact| per output array in units of 2^-53 -- cd_ekf 500, cd_eks 2e3, cd_sgp_filter 500,
cd_sgp_smoother 1e3 -- for the NumPy timed oracle here and for the kernels on the GPU, as they are (the untimed GPU tests allow ten times
them; these do not).  A smoother runs on its implementation's own filtering rows, as in tests/test_exact.py.
Measured (pytest -s), worst case of each method: in the docstrings of the two tests."""
import os

import numpy as np
import pytest

from tests import cases as cs
from tests import times_oracle as to

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = 2.0 ** -53
GATE = {'cd_ekf': 500., 'cd_eks': 2e3, 'cd_sgp_filter': 500., 'cd_sgp_smoother': 1e3}
Z = np.load(os.path.join(GOLD, 'exact_timed.npz'))
NAMES = sorted({k.split('.')[0] for k in Z.files if k.endswith('.dts')})


def case(name):
    """-> (tests/cases.py case of the builder, dts, ys, n, skip, exact {method: arrays})"""
    build = name.split('_')[0]
    p = Z[f'{build}.params']
    c = cs.chirp_case(T=8, params=tuple(p), Xi=float(Z['Xi']), dt=float(Z['dt'])) if build == 'chirp' else \
        cs.lascala_case(T=8, params=tuple(p[2:]), Xi=float(Z['Xi']), dt=float(Z['dt']))
    ys = Z[f'{name}.ys']
    exact = {m: tuple(Z[f'{name}.{m}.{i}'] for i in range(3 if 'smoother' not in m and m != 'cd_eks' else 2)) for m in GATE}
    return c, Z[f'{name}.dts'], ys, int(Z[f'{name}.n']), bool(np.isnan(ys).any()), exact


def amplification(got, want):
    return max(cs.max_rel_err(g, w) / EPS for g, w in zip(got, want))


def test_the_fixture_is_what_the_generator_describes():
    assert int(Z['digits']) >= 100 and all(Z[k].dtype == np.float64 for k in Z.files)
    assert NAMES == sorted(f'{b}_{c}' for b in ('chirp', 'lascala') for c in ('jitter', 'zero3x', 'sub3', 'gaps'))
    dt = float(Z['dt'])
    for name in NAMES:
        _, dts, ys, n, skip, exact = case(name)
        assert dts.shape == ys.shape and ys.size <= 40 and (dts >= 0).all()
        assert n == (3 if name.endswith('sub3') else 1) and skip == name.endswith('gaps')
        assert (dts.min() == 0.0 and dts.max() == 3 * dt) == name.endswith('zero3x')
        assert all(np.isfinite(a).all() and a.shape[0] == ys.size for arrays in exact.values() for a in arrays)
    assert np.array_equal(Z['chirp_jitter.dts'], dt * (1.0 + 0.75 * np.random.default_rng(5).uniform(-1.0, 1.0, 32)))
    assert np.array_equal(Z['chirp_jitter.ys'], cs.chirp_case(T=32).ys)


@pytest.mark.parametrize('name', NAMES)
def test_the_numpy_timed_oracle_sits_within_the_gates_of_the_exact_values(name):
    """tests/times_oracle.py -- oracle/np_filters.py one step at a time -- on every case.  Measured, units of 2^-53, worst case of each method:
    cd_ekf 4.6 (lascala_sub3), cd_eks 4.6 (chirp_sub3), cd_sgp_filter 5.3 (chirp_zero3x, lascala_gaps), cd_sgp_smoother 8.0 (chirp_zero3x)."""
    from oracle import np_filters as onp
    c, dts, ys, n, _, exact = case(name)
    sg = cs.osig(cs.chirp_case(T=8).sgps)                                  # Gauss-Hermite order 3, d = 4
    for filt, smoo, ff, sf, b, head in (('cd_ekf', 'cd_eks', onp.cd_ekf, onp.cd_eks, c.o_disp, ()),
                                        ('cd_sgp_filter', 'cd_sgp_smoother', onp.cd_sgp_filter, onp.cd_sgp_smoother, c.o_disp(None), (sg,))):
        kept, full = to.run_filter_substeps(ff, n, c.o_drift, b, *head, c.H, c.Xi, c.m0, c.P0, dts, ys)      # (n = 1: the timed oracle itself, gaps skipped)
        got = {filt: kept, smoo: to.run_smoother_substeps(sf, n, c.o_drift, b, *head, full[0], full[1], dts)}
        for fn in (filt, smoo):
            a = amplification(got[fn], exact[fn])
            print(f'{name} numpy {fn:16s} {a:10.3g} x 2^-53  = {a * EPS:.2e}')
            assert a < GATE[fn], (name, fn, a)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', ['default', 'lane', 'generic-wave'])
@pytest.mark.parametrize('name', NAMES)
def test_the_hip_kernels_sit_within_the_same_gates(name, shape):
    """cgp_filter_timed / cgp_smoother_timed through the Python front ends: the route the call takes (the d = 4 matrix-core kernels), one lane
    per trial and the forced generic wave kernel.  Measured on an MI355X, units of 2^-53, worst case of each method over the three shapes:
    cd_ekf 8.0, cd_eks 22.6, cd_sgp_filter 9.1, cd_sgp_smoother 8.3."""
    from chirpgp_amd import filters_smoothers as fs
    c, dts, ys, n, skip, exact = case(name)
    flags = {'default': 0, 'lane': 0x4, 'generic-wave': 0x12}[shape]
    kw = dict(dts=dts, substeps=n, flags=flags)
    sg = cs.chirp_case(T=8).sgps
    skip_kw = dict(missing='skip') if skip else {}
    got = {}
    got['cd_ekf'] = fs.cd_ekf(c.drift, c.disp, c.H, c.Xi, c.m0, c.P0, None, ys, **kw, **skip_kw)
    got['cd_sgp_filter'] = fs.cd_sgp_filter(c.drift, c.disp(None), sg, c.H, c.Xi, c.m0, c.P0, None, ys, **kw, **skip_kw)
    if not (n > 1 and shape == 'lane'):                       # (substeps run a smoother one wavefront per trial only)
        got['cd_eks'] = fs.cd_eks(c.drift, c.disp, got['cd_ekf'][0], got['cd_ekf'][1], None, **kw)
        got['cd_sgp_smoother'] = fs.cd_sgp_smoother(c.drift, c.disp(None), sg, got['cd_sgp_filter'][0], got['cd_sgp_filter'][1], None, **kw)
    for fn in got:
        a = amplification(got[fn], exact[fn])
        print(f'{name} hip/{shape} {fn:16s} {a:10.3g} x 2^-53  = {a * EPS:.2e}')
        assert a < GATE[fn], (name, shape, fn, a)
