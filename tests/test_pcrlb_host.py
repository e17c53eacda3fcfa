"""CPU tests of the posterior Cramer-Rao feature: the ABI's two entry points, the float64 oracle (tests/pcrlb_oracle.py) against
100-digit arithmetic (tests/golden/exact_pcrlb.npz), the host recursion of chirpgp_amd/crlb.py, and the front end's refusals."""
import os
import re

import numpy as np
import numpy.testing as npt
import pytest

from tests import pcrlb_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'exact_pcrlb.npz')
NAMES = ('chirp', 'nh2', 'nh3', 'm32')


@pytest.fixture(scope='module')
def exact():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def model_of(exact, name):
    return int(exact[f'{name}_id']), int(exact[f'{name}_d']), exact[f'{name}_params'], float(exact[f'{name}_dt'])


def descriptor_of(exact, name):
    from chirpgp_amd import models as M
    mid, d, p, _ = model_of(exact, name)
    if mid == O.M_LINEAR:
        return M.linear_cond_m_cov(p[:d * d].reshape(d, d), p[d * d:].reshape(d, d))
    return M.disc_harmonic_chirp_lcd(p[0], p[1], p[2], p[3], (d - 2) // 2, p[4])


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from chirpgp_amd import _engine
    return _engine.load_library(), _engine


def test_entry_points_are_declared_exported_and_bound():
    lib, eng = _lib()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'chirpgp_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(cgp_[a-z0-9_]+)\s*\(', src))
    assert declared == set(eng.EXPORTS)
    assert 'cgp_pcrlb_sums' in eng.EXPORTS and 'cgp_simulate_x0' in eng.EXPORTS
    for name in ('cgp_pcrlb_sums', 'cgp_simulate_x0'):
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.cgp_version() == 160
    assert callable(eng.run_pcrlb_sums) and callable(eng.run_simulate_x0)
    assert eng.pcrlb_rows(4) == 26 and eng.pcrlb_rows(8) == 100


def test_null_context_is_rejected_without_gpu():
    lib, _ = _lib()
    assert lib.cgp_pcrlb_sums(None, None, 0.1, None, None, 1, 1, None, 0, None) == -1
    assert lib.cgp_simulate_x0(None, None, None, 1, 0, 1, None, None) == -1


@pytest.mark.parametrize('name', NAMES)
def test_oracle_against_100_digits(exact, name):
    """Every array of the fixture, per model: max |oracle - exact| / the array's largest entry, printed and gated at the figure recorded
    in pcrlb_oracle.ORACLE_ERROR (the measurement rounded up to the next power of ten)."""
    mid, d, p, dt = model_of(exact, name)
    xs, xt = exact[f'{name}_xs'], exact[f'{name}_xt']
    got = [O.pair_blocks(mid, d, p, dt, u, x) for u, x in zip(xs, xt)]
    b11, b12 = np.array([g[0] for g in got]), np.array([g[1] for g in got])
    D22 = O.d22(mid, d, p, dt, exact[f'{name}_H'], float(exact[f'{name}_Xi']))
    rec = exact[f'{name}_rec']
    js = O.recursion(b11[rec].mean(axis=1), b12[rec].mean(axis=1), D22, exact[f'{name}_j0'])
    figures = {'b11': rel(b11, exact[f'{name}_b11']), 'b12': rel(b12, exact[f'{name}_b12']), 'js': rel(js, exact[f'{name}_js']),
               'd22': rel(D22, exact[f'{name}_d22'])}
    print(name, {k: f'{v:.2e}' for k, v in figures.items()})
    for key in ('b11', 'b12', 'js'):
        assert figures[key] <= O.ORACLE_ERROR[name][key], (key, figures[key])
    assert figures['d22'] <= O.ORACLE_ERROR[name]['b12']            # D22 = P + a rank-one term: P is b12's only ingredient besides J
    assert np.all(np.isfinite(exact[f'{name}_js']))
    # the fixture covers what it says: the frequency state at all eight points, one pair with r = 0
    if mid == O.M_HARMONIC_LCD:
        assert sorted(set(xs[:, d - 2])) == [-40.0, -1.75, -1.5, 0.0, 1.5, 2.0, 30.0, 650.0]
    m3 = O.mean_jac_hess(mid, d, p, dt, xs[3])[0]
    assert np.max(np.abs(xt[3] - m3)) <= 1e-15 * max(1.0, np.max(np.abs(m3)))


@pytest.mark.parametrize('name', NAMES)
def test_host_recursion_from_exact_blocks(exact, name):
    """crlb.recursion fed the fixture's exact blocks (as the sums a kernel would hand it) against the fixture's 100-digit js, at the
    figure recorded as ORACLE_ERROR[name]['recursion'] (measured here, rounded up to the next power of ten)."""
    from chirpgp_amd import crlb
    _, d, _, dt = model_of(exact, name)
    rec = exact[f'{name}_rec']
    sums = O.pack(exact[f'{name}_b11'][rec].sum(axis=1), exact[f'{name}_b12'][rec].sum(axis=1)).T          # (K, 6) over N = 5 samples
    js = crlb.recursion(sums, 5, exact[f'{name}_j0'], descriptor_of(exact, name), exact[f'{name}_H'], float(exact[f'{name}_Xi']), dt)
    assert js.shape == (6, d, d)
    fig = rel(js, exact[f'{name}_js'])
    print(name, f'{fig:.2e}')
    assert fig <= O.ORACLE_ERROR[name]['recursion']
    npt.assert_allclose(crlb.bound(js) @ js, np.broadcast_to(np.eye(d), js.shape), atol=1e-9)
    d11, d12 = crlb.unpack(sums, 5, d)
    npt.assert_array_equal(d11, np.swapaxes(d11, 1, 2))
    npt.assert_allclose(d12, exact[f'{name}_b12'][rec].mean(axis=1), rtol=1e-15, atol=0)


@pytest.mark.parametrize('name', ('chirp', 'nh3'))
def test_second_order_term_has_zero_mean(exact, name):
    """E[r | x_s] = 0, so the mean of sum_i w_i Hess m_i over 20 000 seeded samples is within 6 standard errors of zero in every entry
    (a residual taken from another mean than the one the samples were drawn from is not)."""
    mid, d, p, dt = model_of(exact, name)
    rng = np.random.default_rng(7)
    P = O.precision_of(mid, d, p, dt)
    L = np.linalg.cholesky(O.sigma_of(mid, d, p, dt))
    n = 20000
    u = rng.normal(size=(n, d))
    x = O.mean_jac_hess(mid, d, p, dt, u)[0] + rng.normal(size=(n, d)) @ L.T
    terms = O.second_order(mid, d, p, dt, P, u, x)
    mean, se = terms.mean(axis=0), terms.std(axis=0, ddof=1) / np.sqrt(n)
    iv = d - 2
    assert np.all(se[:iv, iv] > 0) and se[iv, iv] > 0                  # the entries that can be non-zero are
    assert np.all(np.abs(mean) <= 6 * se), (mean, se)


def test_reference_lgssm_test_on_the_oracle():
    """test/test_crlb.py:21-37, 75-87 with N = 64: for a linear Gaussian model the bound is the Kalman filter's covariance."""
    from chirpgp_amd.tools import lti_sde_to_disc
    ell, sigma, dt, T, N = 1., 1., 0.1, 10, 64
    A = np.array([[0., 1.], [-3 / ell ** 2, -2 * np.sqrt(3) / ell]])
    Bv = np.array([0., 2 * sigma * (np.sqrt(3) / ell) ** 1.5])
    F, Sigma = lti_sde_to_disc(A, Bv, dt)
    Xi, H = 1., np.array([1., 0.])
    P0 = np.diag([sigma ** 2, 3 / ell ** 2 * sigma ** 2])
    rng = np.random.default_rng(666)
    params = np.concatenate([F.ravel(), Sigma.ravel()])
    cs = np.linalg.cholesky(Sigma)
    x0 = rng.normal(size=(N, 2)) @ np.sqrt(P0)
    xs = np.empty((N, T, 2))
    x = x0
    for t in range(T):
        x = x @ F.T + rng.normal(size=(N, 2)) @ cs.T
        xs[:, t] = x
    s = O.sums(O.M_LINEAR, 2, params, dt, x0, xs) / N
    n11 = 3
    il = np.tril_indices(2)
    d11 = np.zeros((T, 2, 2))
    d11[:, il[0], il[1]] = s[:n11].T
    d11[:, il[1], il[0]] = s[:n11].T
    js = O.recursion(d11, s[n11:].T.reshape(T, 2, 2), O.d22(O.M_LINEAR, 2, params, dt, H, Xi), np.linalg.inv(P0))
    P, Pfs = P0, []
    for _ in range(T):                                                  # kf's covariance recursion (filters_smoothers.py:174-181)
        Pp = F @ P @ F.T + Sigma
        S = H @ Pp @ H + Xi
        K = Pp @ H / S
        P = Pp - np.outer(K, K) * S
        Pfs.append(P)
    npt.assert_allclose(np.linalg.inv(js), np.array(Pfs), atol=1e-12)


def test_front_end_refusals():
    from chirpgp_amd import models as M, crlb
    xss, yss, j0, H = np.zeros((4, 5, 4)), np.zeros((3, 5)), np.eye(4), np.array([0., 1., 0., 0.])
    with pytest.raises(TypeError, match='callable'):
        M.posterior_cramer_rao(xss, yss, j0, lambda u, dt: (u, np.eye(4)), H, 0.1, 0.01)
    with pytest.raises(ValueError, match='disc_model_lascala_lcd'):
        M.posterior_cramer_rao(xss, yss, j0, M.disc_model_lascala_lcd(1., 1.), H, 0.1, 0.01)
    drift, _, _, _, _ = M.model_chirp(0.1, 0.1, 1., 1., 0.1)
    with pytest.raises(ValueError, match='SDE drift'):
        M.posterior_cramer_rao(xss, yss, j0, drift, H, 0.1, 0.01)
    chirp = M.disc_chirp_lcd(0.1, 0.1, 1., 1.)
    with pytest.raises(ValueError, match='xss must be'):
        M.posterior_cramer_rao(np.zeros((4, 5, 3)), yss, j0, chirp, H, 0.1, 0.01)
    with pytest.raises(ValueError, match='yss must be'):
        M.posterior_cramer_rao(xss, np.zeros((4, 5)), j0, chirp, H, 0.1, 0.01)
    with pytest.raises(ValueError, match='j0 must be'):
        crlb.recursion(np.zeros((26, 3)), 5, np.eye(3), chirp, H, 0.1, 0.01)
    with pytest.raises(ValueError, match='sums must be'):
        crlb.recursion(np.zeros((25, 3)), 5, j0, chirp, H, 0.1, 0.01)
