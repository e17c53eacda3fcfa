"""The Fisher-information layer on the host side (no GPU): mle.covariance_from_fisher -- the scaled inverse, its singular branch, the delta
method through g -- and the fixture tests/golden/exact_fisher.npz itself: symmetric, positive semi-definite, and reproduced by a float64
NumPy restatement of the EKF's formula F = sum_t (d nu d nu^T / S + d S d S^T / (2 S^2)) with complex-step tangents, which guards the
100-digit generator (tests/golden/make_exact_fisher.py) against a slip of its own."""
import os
import re

import numpy as np
import numpy.testing as npt
import pytest

from chirpgp_amd import mle

HERE = os.path.dirname(os.path.abspath(__file__))
ZF = np.load(os.path.join(HERE, 'golden', 'exact_fisher.npz'))
ZG = np.load(os.path.join(HERE, 'golden', 'exact_grad_cases.npz'))
NAMES = [str(n) for n in ZF['names']]


def test_covariance_from_fisher_by_hand():
    """F = D^1/2 C D^1/2 with units eight orders apart: cov = F^-1, se = sigmoid(theta) sqrt(diag cov), cond is that of the SCALED matrix."""
    C = np.array([[1.0, 0.5, 0.0], [0.5, 1.0, 0.25], [0.0, 0.25, 1.0]])
    d = np.array([1e-4, 1.0, 1e4])
    F = C * np.sqrt(d)[:, None] * np.sqrt(d)[None, :]
    theta = np.array([-2.0, 0.0, 3.0])
    se, cov, cond, singular = mle.covariance_from_fisher(F, theta)
    assert not singular
    # C^-1 by cofactors: det C = 1 - 0.0625 - 0.25 = 0.6875
    Cinv = np.array([[0.9375, -0.5, 0.125], [-0.5, 1.0, -0.25], [0.125, -0.25, 0.75]]) / 0.6875
    want = Cinv / (np.sqrt(d)[:, None] * np.sqrt(d)[None, :])
    npt.assert_allclose(cov, want, rtol=1e-13)
    npt.assert_allclose(cov @ F, np.eye(3), atol=1e-9)
    npt.assert_allclose(cond, np.linalg.cond(C), rtol=1e-12)
    assert cond < 10.0 < np.linalg.cond(F)
    npt.assert_allclose(se, np.sqrt(np.diag(want)) / (1.0 + np.exp(-theta)), rtol=1e-13)
    npt.assert_array_equal(cov, cov.T)


def test_a_singular_information_is_flagged_not_inverted():
    """A rank-2 matrix: inf in every entry and the flag, where a pseudo-inverse would report a small error along the flat direction."""
    u, v = np.array([1.0, 2.0, -1.0]), np.array([0.5, -1.0, 3.0])
    F = np.outer(u, u) + np.outer(v, v)
    se, cov, cond, singular = mle.covariance_from_fisher(F, np.zeros(3))
    assert singular and np.all(np.isinf(se)) and np.all(np.isinf(cov))
    assert np.all(np.isfinite(np.linalg.pinv(F)))                 # (what is refused)
    # a zero row (a parameter the likelihood does not see: lam = 0) and a NaN matrix take the same branch
    G = np.diag([1.0, 0.0, 2.0])
    assert mle.covariance_from_fisher(G, np.zeros(3))[3] and mle.covariance_from_fisher(np.full((3, 3), np.nan), np.zeros(3))[3]
    # just on the regular side of 1 / cond = 1e-12
    e = 1e-10
    ok = np.array([[1.0, 1.0 - e], [1.0 - e, 1.0]])
    assert not mle.covariance_from_fisher(ok, np.zeros(2))[3]
    with pytest.raises(ValueError):
        mle.covariance_from_fisher(np.eye(3), np.zeros(2))


def test_the_delta_method_factor():
    """se_params = g'(theta) se_theta with g = softplus: the factor is sigmoid(theta), checked against the difference quotient of models.g."""
    from chirpgp_amd import models as pm
    theta = np.array([-30.0, -3.0, 0.0, 0.5, 40.0])
    F = np.diag([4.0, 0.25, 1.0, 16.0, 100.0])
    se, cov, _, singular = mle.covariance_from_fisher(F, theta)
    assert not singular
    h = 1e-6
    dg = (np.log1p(np.exp(-np.abs(theta + h))) + np.maximum(theta + h, 0) - np.log1p(np.exp(-np.abs(theta - h))) - np.maximum(theta - h, 0)) / (2 * h)
    npt.assert_allclose(se, dg / np.sqrt(np.diag(F)), rtol=1e-8, atol=1e-300)
    npt.assert_allclose(pm.g(theta[1:4]), np.log1p(np.exp(theta[1:4])), rtol=1e-14)


def test_scoring_step_and_a_parameter_the_likelihood_does_not_see():
    """(F + mu diag F) step = -grad; a zero row of F (with it the matrix is singular for every mu) leaves that parameter where it is,
    whatever its gradient entry, and gives the others the step of the system without it."""
    F = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, -1.0], [0.5, -1.0, 2.0]])
    g = np.array([1.0, -2.0, 0.5])
    for mu in (0.0, 1e-3, 7.0):
        step = mle.scoring_step(F, g, mu)
        npt.assert_allclose((F + mu * np.diag(np.diag(F))) @ step, -g, rtol=1e-13)
    npt.assert_allclose(mle.scoring_step(F, g, 1e9), -g / (1e9 * np.diag(F)), rtol=1e-8)     # heavy damping: scaled steepest descent
    Z = np.zeros((4, 4))
    Z[np.ix_([0, 1, 3], [0, 1, 3])] = F
    gz = np.array([1.0, -2.0, 5.0, 0.5])
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.solve(Z + 1e-3 * np.diag(np.diag(Z)), -gz)
    step = mle.scoring_step(Z, gz, 1e-3)
    assert step[2] == 0.0
    npt.assert_array_equal(step[[0, 1, 3]], mle.scoring_step(F, g, 1e-3))
    npt.assert_array_equal(mle.scoring_step(np.zeros((2, 2)), np.ones(2), 1.0), 0.0)


def test_the_fixture_holds_what_it_must():
    """At least 18 of the 22 cases, one of every line of the generator's list, the admitted ones within its movement rule."""
    from tests.golden import make_exact_fisher as gen
    assert len(NAMES) >= gen.MIN_CASES and len(NAMES) + len(ZF['rejected']) == sum(len(line) for line in gen.CASES)
    for line in gen.CASES:
        assert set(line) & set(NAMES), line
    for n in NAMES:
        assert n.startswith('edge_') or float(ZF[f'{n}.moved_fisher']) < gen.FISHER_MOVE_MAX, n
        assert ZF[f'{n}.fisher'].shape == (int(ZF[f'{n}.n_dir']),) * 2
    print('rejected:', dict(zip([str(n) for n in ZF['rejected']], ZF['rejected_moved'])))


@pytest.mark.parametrize('name', NAMES)
def test_fixture_matrices_are_symmetric_and_psd(name):
    F = ZF[f'{name}.fisher']
    scale = np.abs(F).max()
    assert np.abs(F - F.T).max() <= 1e-12 * scale
    assert np.linalg.eigvalsh(0.5 * (F + F.T)).min() >= -1e-12 * scale


def _ekf_fisher_numpy(c, T):
    """The EKF of filters_smoothers.py:222-264 on the chirp / La Scala model in complex float64: theta_k (or Xi) + i h, and the imaginary
    parts of nu_t and S_t over h are their tangents -- the constants from mle's complex-safe builders, the state-dependent part here."""
    from chirpgp_amd import models as pm
    consts = mle._constants_of(pm.build_chirp_model if c['build'] == 'chirp' else pm.build_lascala_model)
    theta, dt, H, ys = c['theta'], c['dt'], c['H'].astype(np.complex128), c['ys'][:T]
    nd = theta.size + c['with_dxi']
    h = 1e-30
    dnu, dS, S0 = np.zeros((nd, T)), np.zeros((nd, T)), np.zeros(T)
    for k in range(nd):
        th = theta.astype(np.complex128)
        Xi = complex(c['Xi'])
        if k < theta.size:
            th[k] += 1j * h
        else:
            Xi += 1j * h
        k_ = consts(np.log1p(np.exp(th))[:, None], dt, Xi)[:, 0]
        rho, q, M, MS = np.exp(k_[0]), k_[1], k_[2:6], k_[6:9]
        m = k_[10:14].copy()
        P = np.zeros((4, 4), dtype=np.complex128)
        P[np.tril_indices(4)] = k_[14:24]
        P = P + np.tril(P, -1).T
        Sig = np.zeros((4, 4), dtype=np.complex128)
        Sig[0, 0] = Sig[1, 1] = q
        Sig[2, 2], Sig[2, 3], Sig[3, 2], Sig[3, 3] = MS[0], MS[1], MS[1], MS[2]
        for t in range(T):
            sp, dsp = np.log1p(np.exp(m[2])), 1.0 / (1.0 + np.exp(-m[2]))
            ang = 2 * np.pi * dt * sp
            rc, rs, th1 = rho * np.cos(ang), rho * np.sin(ang), 2 * np.pi * dt * dsp
            mp = np.array([rc * m[0] - rs * m[1], rs * m[0] + rc * m[1], M[0] * m[2] + M[1] * m[3], M[2] * m[2] + M[3] * m[3]])
            J = np.array([[rc, -rs, -th1 * mp[1], 0], [rs, rc, th1 * mp[0], 0], [0, 0, M[0], M[1]], [0, 0, M[2], M[3]]])
            Pp = J @ P @ J.T + Sig
            PH = Pp @ H
            S = H @ PH + Xi
            nu = ys[t] - H @ mp
            K = PH / S
            m, P = mp + K * nu, Pp - np.outer(K, K) * S
            dnu[k, t], dS[k, t], S0[t] = nu.imag / h, S.imag / h, S.real
    return (dnu / S0) @ dnu.T + (dS / (2 * S0 ** 2)) @ dS.T


@pytest.mark.parametrize('name', [n for n in NAMES if str(ZG[f'{ZF[n + ".source"]}.method']) == 'ekf' and not n.startswith('edge_')])
def test_a_float64_restatement_of_the_formula_agrees(name):
    """Within 1e-6 of the matrix's scale: what a float64 EKF carries on these well-conditioned cases is orders below that, a slip in the
    generator (a wrong step, a transposed index, a missing 1 / 2) is orders above."""
    src = str(ZF[f'{name}.source'])
    c = dict(theta=ZG[f'{src}.theta'], ys=ZG[f'{src}.ys'], Xi=float(ZG[f'{src}.Xi']), dt=float(ZG[f'{src}.dt']), H=ZG[f'{src}.H'],
             build=str(ZG[f'{src}.build']), with_dxi=int(ZG[f'{src}.with_dxi']))
    want = ZF[f'{name}.fisher']
    got = _ekf_fisher_numpy(c, int(ZF[f'{name}.T']))
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f'{name}: float64 restatement against the fixture {err:.2e} of its scale {np.abs(want).max():.3g}')
    assert err < 1e-6


def test_the_entry_points_are_declared_and_exported():
    """Both names in the header (with the fisher argument after grad), in _engine.EXPORTS, and the limit stated once on each side."""
    from chirpgp_amd import _engine as eng
    src = open(os.path.join(os.path.dirname(HERE), 'include', 'chirpgp_hip.h')).read()
    for name in ('cgp_ekf_nll_fisher', 'cgp_sgp_nll_fisher'):
        assert re.search(r'\bint\s+%s\s*\([^;]*double\*\s*grad,\s*double\*\s*fisher,' % name, src)
        assert name in eng.EXPORTS
    assert int(re.search(r'#define\s+CGP_FISHER_MAX_DIR\s+(\d+)', src).group(1)) == eng.FISHER_MAX_DIR == 16
    assert re.search(r'#define\s+CGP_VERSION\s+160\b', src)
