"""The gapped oracle (tests/gap_oracle.py) is what it claims to be: for the linear model its rows are the Gaussian conditioning of the state
on the OBSERVED samples alone, computed here without any recursion, and on a record without NaN it is the oracle itself, bit for bit."""
import numpy as np
import pytest

from oracle import np_filters as onp
from tests import gap_oracle as go
from tests.cases import chirp_case, kpt_case, max_rel_err, osig

T = 14
GAPS = ((0, 1), (3, 6), (9, 10), (13, 14))          # steps 0, 3-5, 9, 13: the first and the last step among them


def _linear_model(d, seed):
    rng = np.random.default_rng(seed)
    F = 0.9 * np.linalg.qr(rng.standard_normal((d, d)))[0] + 0.05 * rng.standard_normal((d, d))
    A = rng.standard_normal((d, d)); Sigma = A @ A.T / d + 0.1 * np.eye(d)
    A = rng.standard_normal((d, d)); P0 = A @ A.T / d + 0.5 * np.eye(d)
    return F, Sigma, rng.standard_normal(d), 0.3, rng.standard_normal(d), P0, rng.standard_normal(T)


def _dense_conditioning(F, Sigma, H, Xi, m0, P0, ys):
    """(mfs, Pfs, cumulative nll) of the linear-Gaussian model by conditioning the joint Gaussian of (x_0 .. x_{T-1}) on the finite ys[: k + 1]."""
    d, n = m0.size, ys.size
    mu, C = np.zeros((n, d)), np.zeros((n, n, d, d))
    m, P = m0, P0
    for k in range(n):
        m, P = F @ m, F @ P @ F.T + Sigma              # the filters predict first: x_0 = F x_{-1} + q, x_{-1} ~ N(m0, P0)
        mu[k], C[k, k] = m, P
        for j in range(k + 1, n):
            C[j, k] = F @ C[j - 1, k]
            C[k, j] = C[j, k].T
    mfs, Pfs, nll = np.zeros((n, d)), np.zeros((n, d, d)), np.zeros(n)
    for k in range(n):
        obs = [t for t in range(k + 1) if np.isfinite(ys[t])]
        if not obs:
            mfs[k], Pfs[k] = mu[k], C[k, k]
            continue
        Cyy = np.array([[H @ C[a, b] @ H for b in obs] for a in obs]) + Xi * np.eye(len(obs))
        Cxy = np.stack([C[k, a] @ H for a in obs], axis=1)                       # d x |obs|
        r = ys[obs] - mu[obs] @ H
        mfs[k] = mu[k] + Cxy @ np.linalg.solve(Cyy, r)
        Pfs[k] = C[k, k] - Cxy @ np.linalg.solve(Cyy, Cxy.T)
        nll[k] = 0.5 * (np.linalg.slogdet(2 * np.pi * Cyy)[1] + r @ np.linalg.solve(Cyy, r))
    return mfs, Pfs, nll


@pytest.mark.parametrize('d', (1, 2, 4, 5))
def test_gapped_kf_is_dense_conditioning_on_the_observed_samples(d):
    F, Sigma, H, Xi, m0, P0, ys = _linear_model(d, 100 + d)
    ys = go.with_gaps(ys, GAPS)
    got = go.gapped(onp.kf, F, Sigma, H, Xi, m0, P0, ys)
    want = _dense_conditioning(F, Sigma, H, Xi, m0, P0, ys)
    for g, w, what in zip(got, want, ('mfs', 'Pfs', 'nll')):
        err = max_rel_err(g, w)
        print(f'd = {d} {what}: {err:.2e}')
        assert err <= 1e-12, (d, what, err)
    inc = np.diff(np.concatenate([[0.0], got[2]]))
    assert np.all(inc[np.isnan(ys)] == 0.0) and np.all(inc[np.isfinite(ys)] != 0.0)


def test_gapped_oracle_without_gaps_is_the_oracle():
    F, Sigma, H, Xi, m0, P0, ys = _linear_model(4, 7)
    for g, w in zip(go.gapped(onp.kf, F, Sigma, H, Xi, m0, P0, ys), onp.kf(F, Sigma, H, Xi, m0, P0, ys)):
        assert np.array_equal(g, w)
    c = chirp_case(T=40)
    for fn, args in ((onp.ekf, (c.o_disc, c.H, c.Xi, c.m0, c.P0, c.dt, c.ys)),
                     (onp.sgp_filter, (c.o_disc, osig(c.sgps), c.H, c.Xi, c.m0, c.P0, c.dt, c.ys)),
                     (onp.cd_ekf, (c.o_drift, c.o_disp, c.H, c.Xi, c.m0, c.P0, c.dt, c.ys))):
        for g, w in zip(go.gapped(fn, *args), fn(*args)):
            assert np.array_equal(g, w), fn.__name__
    k = kpt_case(T=40)
    args = (k.F, k.Sigma, k.o_h, k.Xi, k.m0, k.P0, k.dt, k.ys)
    for g, w in zip(go.gapped_ekf_for_kpt(*args), onp.ekf_for_kpt(*args)):
        assert np.array_equal(g, w)
    assert onp._linear_update is go._linear_update                             # the patch does not outlive a call
