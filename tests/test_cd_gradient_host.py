"""The host half of cgp_cd_ekf_nll_grad, without a GPU: the entry point is declared, exported and bound; mle.has_exact_gradient admits
exactly what is built; mle.tangent_directions_cd -- d (27 constants of the continuous model) / d theta_k -- against the central difference
of the same constants in 100-digit arithmetic; a float64 NumPy restatement of the recursion with its forward tangents
(tests/cd_grad_oracle.py) against every case of the 100-digit fixture tests/golden/exact_cd_grad.npz, at the gates the kernel is held to
(tests/test_gpu_cd_gradient.py) -- float64 reaches them before the GPU is asked to; and the fixture holds what it must.

RESULTS (printed by the tests, none of them set a gate): the restatement's worst value error over the fixture 5.0e-15 (random_cd_14),
worst gradient error 1.7e-14 of its scale (random_cd_11); the record lengths of the GPU test: <= 6.9e-16 / 5.2e-15; tangent_directions_cd: <= 1.3e-15
over both sweeps."""
import re

import numpy as np
import pytest
from mpmath import mp, mpf

from tests import cd_grad_oracle as co
from tests.cd_grad_cases import ENTRY, GRAD_MOVE_MAX, NAMES, PREFIX_T, VALUE_MOVE_MAX, Z, case, errors, gates
from tests.golden.make_exact import g as g_mp
from tests.test_gradient_directions import g_inv, sweep

DIRECTION_GATE = 1e-12
CD_NAMES = ['lam', 'gam'] + [f'Gamma_{k}' for k in range(10)] + ['Xi', 'm0_0', 'm0_1', 'm0_2', 'm0_3'] + [f'P0_{k}' for k in range(10)]


# ------------------------------------------------------------------------------------------------ 1. declared, exported, bound
def test_the_entry_point_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from chirpgp_amd import _engine as E
    from tests.test_abi import HEADER
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert re.search(r'\bint\s+' + ENTRY + r'\s*\(', src) and re.search(r'#define\s+CGP_CD_DIR_DOUBLES\s+27\b', src)
    assert ENTRY in E.EXPORTS and E.CD_DIR_DOUBLES == 27
    lib = E.load_library()
    assert lib.cgp_version() == 160
    assert getattr(lib, ENTRY).argtypes is not None and len(getattr(lib, ENTRY).argtypes) == 16
    assert getattr(lib, ENTRY)(None, None, None, 0.0, None, 1, 1, None, 1, 1, None, 1, None, None, 0, None) == -1      # a NULL context: CGP_E_ARG


# ------------------------------------------------------------------------------------------------ 2. what has an exact gradient
def test_has_exact_gradient_admits_what_is_built():
    from chirpgp_amd import mle, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    assert mle.has_exact_gradient('cd_ekf', pm.build_chirp_model, 0.1)
    assert mle.has_exact_gradient('cd_ekf', pm.build_lascala_model, 0.1)
    assert not mle.has_exact_gradient('cd_ekf', pm.build_chirp_model, np.array([0.1, 0.2]))          # a per-trial Xi: the difference form
    assert not mle.has_exact_gradient('cd_ekf', pm.build_harmonic_chirp_model, 0.1)
    assert not mle.has_exact_gradient('cd_sgp_filter', pm.build_chirp_model, 0.1, sgps=SigmaPoints.gauss_hermite(4, 3))
    assert not mle.has_exact_gradient('cd_eks', pm.build_chirp_model, 0.1)
    assert not mle._exact_by_default('cd_ekf', pm.build_chirp_model, 0.1, 10 ** 6, {})                # no default moves
    assert not mle._has_fisher_form('cd_ekf') and mle._has_fisher_form('ekf') and mle._has_fisher_form('sgp_filter')
    assert re.search('tangent kernel', str(mle._fisher_unsupported('cd_ekf'))) and re.search('tangent kernel', str(mle._exact_unsupported()))


# ------------------------------------------------------------------------------------------------ 3. the directions
def constants_cd_mp(params, Xi, lascala):
    """The 27 constants (include/chirpgp_hip.h: CGP_CD_DIR_DOUBLES) in mpf: models.py:437-459 / 497-519 with 76-119."""
    if lascala:
        delta, ell, sigma, m0_v = params
        lam, b = mpf(0), mpf(0)
    else:
        lam, b, delta, ell, sigma, m0_v = params
    z, gam = mpf(0), mp.sqrt(3) / ell
    disp33 = 2 * sigma * gam ** mpf('1.5')                              # the dispersion's last diagonal entry (models.py:112-113)
    return [lam, gam, b * b, z, b * b, z, z, z, z, z, z, disp33 * disp33, Xi, z, z, m0_v, z, delta, z, delta, z, z, sigma ** 2, z, z, z, gam ** 2 * sigma ** 2]


def exact_directions_cd(theta, Xi, lascala):
    """d constants / d theta (P, 27) and the constants (27,): central differences, step 1e-30, at 100 digits (1200 below theta = -200), as
    tests/test_gradient_directions.py takes the discrete constants'."""
    P = len(theta)
    out = np.empty((P, 27))
    with mp.workdps(1200 if np.min(theta) < -200. else 100):
        h = mpf(10) ** -30
        th, Xim = [mpf(float(t)) for t in theta], mpf(float(Xi))
        for k in range(P):
            tp, tm = list(th), list(th)
            tp[k] += h
            tm[k] -= h
            cp, cm = constants_cd_mp([g_mp(t) for t in tp], Xim, lascala), constants_cd_mp([g_mp(t) for t in tm], Xim, lascala)
            out[k] = [float((a - b_) / (2 * h)) for a, b_ in zip(cp, cm)]
        return out, np.array([float(v) for v in constants_cd_mp([g_mp(t) for t in th], Xim, lascala)])


def rk4_stable(p, dt, lascala):
    """The part of the sweep cd_ekf can run: 2 (sqrt(3) / ell) dt and lam dt below 1."""
    ell, lam = (p[1], 0.) if lascala else (p[3], p[0])
    return 2 * np.sqrt(3.) / ell * dt < 1. and lam * dt < 1.


@pytest.mark.parametrize('lascala', [False, True], ids=['chirp', 'lascala'])
def test_directions_against_100_digits(lascala):
    """tests/test_gradient_directions.py's 200 seeded parameter vectors per builder (lam 1e-12 .. 10 and exactly 0, b 1e-4 .. 10, delta
    1e-3 .. 10, ell 1e-2 .. 100, sigma 1e-2 .. 10, both dt), limited to the RK4-stable part; its metric: |got - exact| / max(|exact|,
    1e-6 |c| sigmoid(theta_k)), an entry whose exact value is 0 must be exactly 0."""
    from chirpgp_amd import mle, models as pm
    build = pm.build_lascala_model if lascala else pm.build_chirp_model
    cases = [c for c in sweep(2024, 200, lascala) if rk4_stable(c[0], c[1], lascala)]
    assert len(cases) >= 120
    worst = (0., None, None, None)
    for i, (p, dt, Xi) in enumerate(cases):
        theta = g_inv(p)
        got = mle.tangent_directions_cd(build, theta[None, :], dt, Xi)[0]
        assert got.shape == (theta.size, 27)
        want, c = exact_directions_cd(theta, Xi, lascala)
        with np.errstate(over='ignore'):
            sig = 1.0 / (1.0 + np.exp(-theta))
        den = np.maximum(np.abs(want), 1e-6 * np.abs(c)[None, :] * sig[:, None])
        with np.errstate(all='ignore'):
            err = np.where(want == 0., np.where(got == 0., 0., np.inf), np.abs(got - want) / np.where(den > 0, den, 1.))
        err = np.where(np.isfinite(got), err, np.inf)
        k, e = np.unravel_index(np.argmax(err), err.shape)
        if err[k, e] > worst[0]:
            worst = (float(err[k, e]), i, int(k), CD_NAMES[e])
    print(f'worst entry error over {len(cases)} RK4-stable vectors: {worst[0]:.2e} (case {worst[1]}, d {worst[3]} / d theta_{worst[2]})')
    assert worst[0] < DIRECTION_GATE, worst


def test_directions_match_the_restatements_analytic_ones():
    """The complex-step directions and the analytic derivatives tests/cd_grad_oracle.py takes are two derivations of the same numbers."""
    from chirpgp_amd import mle, models as pm
    for name in ('prefix_cd_chirp', 'prefix_cd_lascala', 'edge_cd_lam0'):
        c = case(name)
        d = mle.tangent_directions_cd(pm.build_chirp_model if c['build'] == 'chirp' else pm.build_lascala_model, c['theta'][None, :], c['dt'], c['Xi'])[0]
        k = co.constants(c['build'], c['theta'], c['Xi'])
        tri = np.tril_indices(4)
        want = np.concatenate([k['dlam'][:, None], k['dgam'][:, None], k['dGamma'][:, tri[0], tri[1]], k['dXi'][:, None], k['dm0'], k['dP0'][:, tri[0], tri[1]]], axis=1)
        np.testing.assert_allclose(d, want, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------ 4. float64 reaches the gates
def _oracle(c, T=None):
    f, grad = co.value_and_grad(c['build'], c['theta'], c['ys'] if T is None else c['ys'][:T], c['Xi'], c['dt'], H=c['H'],
                                with_dxi=bool(c['with_dxi']), skip_missing=bool(c['skip']))
    return f, grad


@pytest.mark.parametrize('name', NAMES)
def test_float64_restatement_meets_the_gates(name):
    """Every kept case of the fixture: value within 1e-11 relative, gradient within 1e-8 of its largest component (exempt cases:
    max(gate, 100 x the stored movement)); the prefix cases at every record length of the GPU test as well."""
    c = case(name)
    f, grad = _oracle(c)
    value_gate, grad_gate = gates(c)
    ev, eg = errors(f[-1], grad[-1], c['nll'], c['grad'], name)
    assert ev < value_gate and eg < grad_gate, (f[-1], c['nll'], grad[-1], c['grad'])
    if c['group'] == 'prefix':
        want_f, want_g = Z[f'{name}.nll_prefix'], Z[f'{name}.grad_prefix']
        for T in PREFIX_T:
            ev, eg = errors(f[T - 1], grad[T - 1], want_f[T - 1], want_g[T - 1], f'{name} T = {T}')
            assert ev < value_gate and eg < grad_gate, T
    if name == 'gaps_cd_everywhere':
        assert f[-1] == 0.0 and not grad[-1].any()


# ------------------------------------------------------------------------------------------------ 5. the fixture is whole
def test_the_fixture_is_whole():
    counts = {g_: sum(str(Z[f'{n}.group']) == g_ for n in NAMES) for g_ in ('prefix', 'random_cd', 'edge', 'other', 'gaps')}
    for g_, n in counts.items():
        assert int(Z[f'count.{g_}']) == n and n > 0, g_
    assert counts['prefix'] == 2 and counts['gaps'] == 6 and counts['edge'] == 2 and counts['other'] == 1
    assert 6 * counts['random_cd'] >= 5 * 16                                                     # at least 5 of every 6 slots
    assert int(Z['drawn.random_cd']) - int(Z['rejected.random_cd']) == counts['random_cd']
    cases = [case(n) for n in NAMES]
    rnd = [c for c in cases if c['group'] == 'random_cd']
    assert {c['build'] for c in rnd} == {'chirp', 'lascala'} and {c['dt'] for c in rnd} == {1e-3, 1e-2} and {c['lost'] for c in rnd} == {0, 1}
    assert all(40 <= c['ys'].size <= 130 for c in rnd)
    for c in cases:
        assert c['method'] == 'cd_ekf'
        if c['group'] != 'edge':                                                                 # admitted: under the admission limits
            assert c['moved_nll'] < VALUE_MOVE_MAX and c['moved_grad'] < GRAD_MOVE_MAX, c['name']
        assert np.isfinite(c['moved_nll']) and np.isfinite(c['moved_grad'])
        assert bool(c['skip']) == bool(np.isnan(c['ys']).any()) == (c['group'] == 'gaps')
        # RK4 inside its stability region
        p = np.logaddexp(0., c['theta'])
        ell, lam = (p[3], p[0]) if c['build'] == 'chirp' else (p[1], 0.)
        assert 2 * np.sqrt(3.) / ell * c['dt'] < 1. and lam * c['dt'] < 1., c['name']
    for n in ('prefix_cd_chirp', 'prefix_cd_lascala'):
        assert Z[f'{n}.nll_prefix'].shape == (130,) and Z[f'{n}.grad_prefix'].shape == (130, Z[f'{n}.theta'].size)
        assert Z[f'{n}.nll_prefix'][-1] == Z[f'{n}.nll'] and np.array_equal(Z[f'{n}.grad_prefix'][-1], Z[f'{n}.grad'])
    assert Z['edge_cd_lam0.theta'][0] == -800. and Z['edge_cd_lam0.grad'][0] == 0.
    assert np.logaddexp(0., Z['edge_cd_ell30.theta'][3]) == pytest.approx(30.)
    assert Z['other_cd_H_dXi.grad'].size == 7 and not np.array_equal(Z['other_cd_H_dXi.H'], [0., 1., 0., 0.])
    ys = {n: Z[f'gaps_cd_{n}.ys'] for n in ('first', 'last', 'run', 'everywhere')}
    assert np.isnan(ys['first'][0]) and np.isnan(ys['last'][-1]) and np.isnan(ys['run'][5:12]).all() and np.isnan(ys['everywhere']).all()
    assert Z['gaps_cd_everywhere.nll'] == 0.0 and not Z['gaps_cd_everywhere.grad'].any()
