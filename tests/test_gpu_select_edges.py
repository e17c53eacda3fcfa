"""The Gauss-Hermite epilogue of the smoothers (csrc/cgp_kernels.hpp: gh_expectation) at the edges of its three tiers -- every node at or
above 6 (lean exponential), any node within (-700, 700) (the branch-free softplus), otherwise the library -- which the smoothers' own
rows never visit: hand-made filtering rows at T = 1 and T = 2, whose last smoothing row is the last filtering row, so that (m, sqrt(v))
is whatever the test sets.  Reference: the rule's own weighted sum of softplus at its nodes in 200-bit arithmetic -- the nodes being the
doubles x_p = fma(s, xi_p, m) that a float64 rule has (at x = -698 half an ulp of x is 6e-14 of exp(x): against the unrounded m + s xi_p no
float64 evaluation could hold a gate made of roundings of the terms; measured so, the branch-free tier sat at 3.4 gates there, all of it
the argument's).  Gates: (order + 4) roundings
of the sum's terms plus 2e-15 of the value (the branch-free softplus's gate); in the first tier the lean exponential's measured error on
sum w_p exp(-x_p) more.  And the header's promise: a trial's value does not depend on the trials it shares a wavefront with."""
import functools

import mpmath as mp
import numpy as np
import pytest

from tests import cases as cs
from tests import fastmath_points as fp

pytestmark = pytest.mark.gpu

WAVE, LANE, GENERIC = 0x2, 0x4, 0x10
ORDERS = (1, 7, 32)


def _rule(order):
    from chirpgp_amd import _engine as E
    return E._gh_rule(order)


def _reach(order, s):
    """as the kernel forms it: the largest |node|, times |s|, in float64"""
    return np.abs(_rule(order)[0]).max() * np.abs(s)


def _tier(order, m, s):
    """the tier gh_expectation picks for a lane, in the kernel's own float64 comparisons (0: NaN)"""
    reach = _reach(order, s)
    with np.errstate(invalid='ignore'):
        t1 = (m - reach >= 6.0) & (m + reach < 700.0)
        t2 = ~t1 & (m - reach > -700.0) & (m + reach < 700.0)
    return np.where(np.isnan(m) | np.isnan(s), 0, np.where(t1, 1, np.where(t2, 2, 3)))


@functools.lru_cache(maxsize=None)
def _trials(order, B):
    """(m, s) of B trials: the tier edges first -- m - reach at 6 and at -700, m + reach at 700, each with the two doubles either side, for
    a narrow and a wide fan; v = 0 -- then regular trials, and one NaN trial.  Every s has 26 significant bits at most: v = s^2 and sqrt(v) = s
    are exact."""
    pts = []
    for s in ((0.0,) if order == 1 else (0.5, 3.0)):
        reach = float(_reach(order, s))
        for m0 in (6.0 + reach, 700.0 - reach, -700.0 + reach):
            pts += [(float(fp.nudge(m0, n)), s) for n in (-2, -1, 0, 1, 2)]
    pts += [(3.25, 0.0), (6.0, 0.0), (float(fp.nudge(6.0, -1)), 0.0), (40.0, 0.0), (700.0, 0.0), (float(fp.nudge(700.0, -1)), 0.0), (-700.0, 0.0),
            (float(fp.nudge(-700.0, 1)), 0.0), (-30.0, 0.0)]
    rng = np.random.default_rng(100 * order + B)
    fill = B - len(pts) - 1
    assert fill > 0
    reg_m = rng.uniform(-5.0, 20.0, fill)
    reg_s = np.round(rng.uniform(0.0, 1.0, fill) * 2 ** 20) / 2 ** 20
    m = np.concatenate([[p[0] for p in pts], reg_m])
    s = np.concatenate([[p[1] for p in pts], reg_s])
    nan_at = 41 if B > 41 else B - 1
    m, s = np.insert(m, nan_at, np.nan), np.insert(s, nan_at, 0.5)
    assert m.size == B
    return m, s


@functools.lru_cache(maxsize=None)
def _reference(order, B):
    """per trial: the rule's weighted sum at 200 bits (as hi + lo), its gate, its tier"""
    m, s = _trials(order, B)
    xi, w = _rule(order)
    tier = _tier(order, m, s)
    eps_exp = fp.measure('exp_lean')
    hi, lo, gate = np.full(B, np.nan), np.zeros(B), np.full(B, np.nan)
    with mp.workprec(fp.PREC):
        for b in range(B):
            if tier[b] == 0:
                continue
            # the rule's nodes are doubles: fma(s, xi_p, m), one rounding (float() of the exact value rounds it the same way)
            x = [mp.mpf(float(mp.mpf(float(m[b])) + mp.mpf(float(s[b])) * mp.mpf(float(z)))) for z in xi]
            f = [mp.log1p(mp.exp(v)) for v in x]
            total = mp.fsum(mp.mpf(float(wp)) * fv for wp, fv in zip(w, f))
            g = (order + 4) * mp.ldexp(1, -53) * mp.fsum(abs(mp.mpf(float(wp)) * fv) for wp, fv in zip(w, f)) + mp.mpf('2e-15') * abs(total)
            if tier[b] == 1:
                g += mp.mpf(eps_exp) * mp.fsum(mp.mpf(float(wp)) * mp.exp(-v) for wp, v in zip(w, x))
            hi[b] = float(total)
            lo[b] = float(total - mp.mpf(hi[b]))
            gate[b] = float(g)
    return hi, lo, gate, tier


def _rows(d, comp, m, s, T):
    """filtering rows whose LAST row has mean m and variance s^2 in component comp; the rows before it are ordinary ones"""
    B = m.size
    mfs = np.zeros((B, T, d))
    Pfs = np.tile(0.01 * np.eye(d), (B, T, 1, 1))
    mfs[:, :, comp] = 8.0
    mfs[:, T - 1, comp] = m
    Pfs[:, T - 1, comp, comp] = s * s
    return mfs, Pfs


@functools.lru_cache(maxsize=None)
def _case(d):
    return cs.chirp_case(T=4, seed=3) if d == 4 else cs.harmonic_case(T=4, seed=58, nh=3)


def _expect(d, flags, order, m, s, T, want=(False, False)):
    from chirpgp_amd import filters_smoothers as fs
    c = _case(d)
    mfs, Pfs = _rows(d, d - 2, m, s, T)
    out = fs.eks(c.disc, mfs, Pfs, c.dt, flags=flags, want=want, select=dict(comp=-2, expect='softplus', order=order))
    return np.asarray(out[2]['expect'])[:, T - 1]


def _check(got, order, B, what):
    hi, lo, gate, tier = _reference(order, B)
    live = tier > 0
    assert np.isnan(got[~live]).all() and (~live).sum() == 1, what
    assert np.isfinite(got[live]).all(), (what, _trials(order, B)[0][live][~np.isfinite(got[live])])
    err = np.abs((got[live] - hi[live]) - lo[live])
    ratio = err / gate[live]
    i = int(np.argmax(ratio))
    m, s = _trials(order, B)
    print(f'WORST | gh_expectation, {what} | {ratio[i]:.2e} of its gate ({err[i]:.2e}) | m = {m[live][i]!r}, s = {s[live][i]!r}, tier {tier[live][i]}')
    assert np.all(err <= gate[live]), (what, m[live][err > gate[live]][:5], s[live][err > gate[live]][:5], tier[live][err > gate[live]][:5], ratio.max())
    return got


def test_the_points_sit_on_the_tier_edges():
    """(no launch) the edge trials straddle each comparison of the kernel in its own arithmetic: both verdicts occur among the five doubles"""
    for order in ORDERS:
        m, s = _trials(order, 130)
        tier = _tier(order, m, s)
        assert set(tier) == {0, 1, 2, 3}
        for k in range(0, 15 if order == 1 else 30, 5):
            assert len(set(tier[k:k + 5])) == 2, (order, k, tier[k:k + 5])
        reach = _reach(order, s)
        assert np.any(m - reach == 6.0) and np.any(m + reach == 700.0) and np.any(m - reach == -700.0)
        assert np.array_equal(np.sqrt(s * s), s)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('B', [64, 65, 130])
def test_one_lane_per_trial_epilogue_at_the_tier_edges(order, B):
    """cgp_lane4.hpp: 64 trials a wavefront, so lanes of all three tiers (and a NaN trial) sit side by side."""
    m, s = _trials(order, B)
    for T in (1, 2):
        _check(_expect(4, LANE, order, m, s, T), order, B, f'one lane per trial, order {order}, B = {B}, T = {T}')


@pytest.mark.parametrize('order', ORDERS)
def test_a_trial_does_not_depend_on_its_neighbours(order):
    """The header's promise: every trial of a mixed batch equals, bit for bit, the same trial launched alone -- and in another batch."""
    m, s = _trials(order, 130)
    mixed = _expect(4, LANE, order, m, s, 1)
    alone = np.concatenate([_expect(4, LANE, order, m[b:b + 1], s[b:b + 1], 1) for b in range(130)])
    np.testing.assert_array_equal(mixed.view(np.uint64), alone.view(np.uint64))
    other = _expect(4, LANE, order, m[::-1].copy(), s[::-1].copy(), 1)[::-1]
    np.testing.assert_array_equal(mixed.view(np.uint64), other.copy().view(np.uint64))


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('family,d,flags,want', [('wave-per-trial walk', 4, WAVE, (False, False)), ('d = 8 tile layout', 8, WAVE, (False, False)),
                                                 ('generic kernel, gathered from its rows', 4, GENERIC | WAVE, (True, False))])
def test_wave_per_trial_epilogues_at_the_tier_edges(family, d, flags, want, order):
    """The epilogue behind the d = 4 walk, the d = 8 tile layout, and the second launch that gathers the selection from full rows."""
    B = 64
    m, s = _trials(order, B)
    for T in (1, 2):
        _check(_expect(d, flags, order, m, s, T, want), order, B, f'{family}, order {order}, T = {T}')
