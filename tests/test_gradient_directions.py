"""The host half of the exact-gradient kernels: mle.tangent_directions -- d (24 model constants) / d theta_k, the directions that
cgp_ekf_nll_grad and cgp_sgp_nll_grad carry through the scan -- against the central difference of the same constants in 100-digit
arithmetic (step 1e-30), ENTRY BY ENTRY, over the parameter region the optimiser visits and not at the fixtures' one point.

Covers (the issue's table): host `mle.tangent_directions` / `_chirp_constants` / `_m32_c` -- the complex step through cancelling formulas
-- everywhere else than lam = b = delta = 0.1, ell = sigma = 1.

Metric: |got - exact| / max(|exact|, 1e-6 |c| sigmoid(theta_k)), c the constant itself (the floor only matters where a derivative changes
sign inside the sweep); an entry whose exact value is 0 must be exactly 0.  Gate 1e-12: a thousand times the 1.7e-15 the well-conditioned
entries show, which a cancellation-free form reaches on all of them.

With the reference's formulas differentiated by the complex step as they stand (`b^2 / (2 lam) (1 - exp(-2 lam dt))`,
`sigma^2 - beta (2 eta + 2 eta^2 + 1)`, `(1 + eta) exp(-eta)`) this file fails: worst entries 5.7e-10 at the fixtures' point,
27 (wrong sign and size) for d q / d theta_lam at lam = 1e-6, 2.2e7 at lam = 1e-9, 8.2e-4 for d M32_Sigma[0] / d theta_sigma at
ell = 30; over the sweep 1.3e13 (chirp, lam = 1.1e-12) and 5.1e-3 (La Scala, ell = 82).  With the forms of mle._m32_c / _decay_ratio: <= 5.2e-16 on the
five rows, <= 3.9e-15 over both sweeps."""
import numpy as np
import pytest
from mpmath import mp, mpf

from tests.golden.make_exact import g as g_mp, m32_solution

GATE = 1e-12
NAMES = ['dlogrho', 'q', 'F00', 'F01', 'F10', 'F11', 'S00', 'S01', 'S11', 'Xi', 'm0_0', 'm0_1', 'm0_2', 'm0_3'] + [f'P0_{k}' for k in range(10)]
# lam, b, delta, ell, sigma, m0_v at dt = 1e-3: the rows measured for the issue
ROWS = [(0.1, 0.1, 0.1, 1., 1., 7.), (1e-3, 0.1, 0.1, 1., 1., 7.), (1e-6, 0.3, 0.1, 1., 1., 7.), (1e-9, 0.3, 0.1, 0.05, 1., 7.),
        (0.1, 0.1, 0.1, 30., 1., 7.)]


def g_inv(p):
    """theta with g(theta) = p in float64; p = 0 exactly is theta = -800 (g underflows to 0 there: the builder's lam == 0 branch)."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide='ignore'):
        return np.where(p == 0., -800., np.where(p > 30., p, np.log(np.expm1(np.minimum(p, 30.)))))


def constants_mp(params, dt, Xi, lascala):
    """The 24 constants (include/chirpgp_hip.h: CGP_DIR_DOUBLES) in mpf: models.py:437-459 / 497-519, 264-311, 61-73.  q is written
    b^2 dt (-expm1(-x) / x), x = 2 lam dt -- the same function as the reference's b^2 / (2 lam) (1 - exp(-2 lam dt)), without a
    numerator that vanishes in 100 digits at lam = exp(-800)."""
    if lascala:
        delta, ell, sigma, m0_v = params
        lam, q = mpf(0), mpf(0)
    else:
        lam, b, delta, ell, sigma, m0_v = params
        x = 2 * lam * dt
        q = b ** 2 * dt * (-mp.expm1(-x) / x)
    F, S = m32_solution(ell, sigma, dt)
    z = mpf(0)
    P0 = [delta, z, delta, z, z, sigma ** 2, z, z, z, (mp.sqrt(3) / ell) ** 2 * sigma ** 2]
    return [-lam * dt, q, F[0][0], F[0][1], F[1][0], F[1][1], S[0][0], S[0][1], S[1][1], Xi, z, z, m0_v, z] + P0


def exact_directions(theta, dt, Xi, lascala):
    """d constants / d theta (P, 24) and the constants (24,), rounded to float64 at the end: central differences, step 1e-30, at 100 digits
    (truncation 1e-60 relative).  A vector with a theta below -200 is taken at 1200 digits: g(theta) = exp(theta) is then below 1e-87
    and would drown, with its increment, in 100."""
    P = len(theta)
    out = np.empty((P, 24))
    dps = 1200 if np.min(theta) < -200. else 100
    for k in range(P):
        with mp.workdps(dps):
            h = mpf(10) ** -30
            th = [mpf(float(t)) for t in theta]
            dtm, Xim = mpf(float(dt)), mpf(float(Xi))
            tp, tm = list(th), list(th)
            tp[k] += h
            tm[k] -= h
            cp = constants_mp([g_mp(t) for t in tp], dtm, Xim, lascala)
            cm = constants_mp([g_mp(t) for t in tm], dtm, Xim, lascala)
            out[k] = [float((a - b_) / (2 * h)) for a, b_ in zip(cp, cm)]
    with mp.workdps(dps):
        c = constants_mp([g_mp(mpf(float(t))) for t in theta], mpf(float(dt)), mpf(float(Xi)), lascala)
        return out, np.array([float(v) for v in c])


def entry_errors(got, theta, dt, Xi, lascala):
    """(P, 24) errors by the metric of the module docstring; an entry that must be exactly 0 and is not counts as inf."""
    want, c = exact_directions(theta, dt, Xi, lascala)
    with np.errstate(over='ignore'):
        sig = 1.0 / (1.0 + np.exp(-np.asarray(theta, dtype=np.float64)))
    den = np.maximum(np.abs(want), 1e-6 * np.abs(c)[None, :] * sig[:, None])
    with np.errstate(all='ignore'):
        err = np.where(want == 0., np.where(got == 0., 0., np.inf), np.abs(got - want) / np.where(den > 0, den, 1.))
    return np.where(np.isfinite(got), err, np.inf)


def sweep(seed, n, lascala):
    """Seeded log-uniform parameter vectors: lam 1e-12 .. 10 and (every eighth) exactly 0, b 1e-4 .. 10, delta 1e-3 .. 10, ell 1e-2 .. 100,
    sigma 1e-2 .. 10, m0_v 0.05 .. 30; dt 1e-3 and 1e-2 alternating; Xi 1e-3 .. 3."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        lam = 0. if i % 8 == 7 else 10 ** rng.uniform(-12, 1)
        b, delta = 10 ** rng.uniform(-4, 1), 10 ** rng.uniform(-3, 1)
        ell, sigma, m0_v = 10 ** rng.uniform(-2, 2), 10 ** rng.uniform(-2, 1), rng.uniform(0.05, 30)
        Xi = 10 ** rng.uniform(-3, np.log10(3.))
        p = (delta, ell, sigma, m0_v) if lascala else (lam, b, delta, ell, sigma, m0_v)
        out.append((np.array(p), 1e-3 if i % 2 == 0 else 1e-2, Xi))
    return out


def worst_errors(tangent_directions, build, cases, lascala):
    """Largest error over the cases and where: (error, case index, parameter k, entry name)."""
    worst = (0., None, None, None)
    for i, (p, dt, Xi) in enumerate(cases):
        theta = g_inv(p)
        got = tangent_directions(build, theta[None, :], dt, Xi)[0]
        err = entry_errors(got, theta, dt, Xi, lascala)
        k, e = np.unravel_index(np.argmax(err), err.shape)
        if err[k, e] > worst[0]:
            worst = (float(err[k, e]), i, int(k), NAMES[e])
    return worst


def _builders():
    from chirpgp_amd import models as pm
    return pm.build_chirp_model, pm.build_lascala_model


@pytest.mark.parametrize('row', range(len(ROWS)))
def test_the_measured_rows(row):
    """The five parameter vectors of the issue's table (chirp builder, dt = 1e-3), every one of the 6 x 24 entries."""
    from chirpgp_amd import mle
    chirp, _ = _builders()
    w = worst_errors(mle.tangent_directions, chirp, [(np.array(ROWS[row]), 1e-3, 0.1)], False)
    print(f'params {ROWS[row]}: worst entry error {w[0]:.2e} (d {w[3]} / d theta_{w[2]})')
    assert w[0] < GATE, w


@pytest.mark.parametrize('lascala', [False, True], ids=['chirp', 'lascala'])
def test_the_parameter_sweep(lascala):
    """200 seeded log-uniform parameter vectors per builder (lam down to 1e-12 and exactly 0, ell 1e-2 .. 100, both dt)."""
    from chirpgp_amd import mle
    build = _builders()[1 if lascala else 0]
    cases = sweep(2024, 200, lascala)
    w = worst_errors(mle.tangent_directions, build, cases, lascala)
    print(f'worst entry error over {len(cases)} vectors: {w[0]:.2e} (case {w[1]}: params {cases[w[1]][0] if w[1] is not None else None}, d {w[3]} / d theta_{w[2]})')
    assert w[0] < GATE, (w, cases[w[1]])


def test_lam_exactly_zero():
    """theta_lam = -800: g underflows to 0, the builder takes its lam == 0 branch.  Every direction is finite, direction 0 is exactly 0
    (sigmoid(-800) = 0) and the others are those of the limit lam -> 0."""
    from chirpgp_amd import mle
    chirp, _ = _builders()
    theta = g_inv(np.array([0., 0.3, 0.1, 1., 1., 7.]))
    assert theta[0] == -800.
    d = mle.tangent_directions(chirp, theta[None, :], 1e-3, 0.1)[0]
    assert np.isfinite(d).all()
    assert np.array_equal(d[0], np.zeros(24))
    near = mle.tangent_directions(chirp, g_inv(np.array([1e-14, 0.3, 0.1, 1., 1., 7.]))[None, :], 1e-3, 0.1)[0]
    np.testing.assert_allclose(d[1:], near[1:], rtol=1e-12, atol=0)
    assert entry_errors(d, theta, 1e-3, 0.1, False).max() < GATE
