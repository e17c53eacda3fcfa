"""The H = e_1 form of the d = 4 matrix-core EKF carries the mean by column only (cgp_mfma4.hpp: Ekf4Anchor): one pair (A2, B2) per
column q is rotated by the angle increment -- forwards in column 0, backwards in column 1, constant in columns 2 / 3 -- and both the
predicted mean f[q] = A2 u[q] + B2 u[q ^ 1] and the matrix operand J0[q][r] are formed from it.  Every tier of the kernel (HIGH, COMMON,
LOW, MID, ANY, wide, checked), records that cross between them, both signs of the increment, lambda = 0, the La Scala model, per-trial
parameters through the four-trials-per-wavefront kernel, an NLL-only launch, a time-split launch and a measurement vector that is not e_1
(the general form, which keeps the mean in both layouts): all against the C port of the reference's recursion at 1e-9 relative to each
output's largest entry, the gate of the full-size parity test."""
import math

import numpy as np
import pytest

from tests import cases as cs

pytestmark = pytest.mark.gpu

GATE = 1e-9
WAVE = dict(flags=0x2)                      # one trial per wavefront: ekf4_mfma_kernel
WAVE_X4 = dict(flags=0x2 | 0x200)           # four trials per wavefront: ekf4_mfma_x4_kernel
NAMES = ('mfs', 'Pfs', 'nll')


def _sweep(f_lo, f_hi, T, seed, Xi=0.05, dt=1e-3, periods=1.5):
    ts = dt * np.arange(1, T + 1)
    freq = f_lo + (f_hi - f_lo) * 0.5 * (1 - np.cos(2 * math.pi * ts / ts[-1] * periods))
    return np.sin(2 * math.pi * np.cumsum(freq) * dt) + math.sqrt(Xi) * np.random.default_rng(seed).standard_normal(T)


def _ramp(f_from, f_to, T, seed, Xi=0.05, dt=1e-3):
    freq = np.linspace(f_from, f_to, T)
    return np.sin(2 * math.pi * np.cumsum(freq) * dt) + math.sqrt(Xi) * np.random.default_rng(seed).standard_normal(T)


def _counted(run):
    from chirpgp_amd import _engine
    _engine.debug_set(_engine.DBG_COUNT_REGIMES, 1)
    _engine.debug_counters(reset=True)
    try:
        got = run()
        return got, _engine.debug_counters(reset=True)
    finally:
        _engine.debug_set(_engine.DBG_COUNT_REGIMES, 0)


def _check(got, want, label):
    errs = [cs.max_rel_err(g, w) for g, w in zip(got, want)]
    print(label, [f'{e:.1e}' for e in errs])
    for e, n in zip(errs, NAMES):
        assert e <= GATE, (label, n, e)


def _tier_records(tier):
    """(model parameters, Xi, records (B, T), what the kernel's own counters must show) for a record set that lives in one tier."""
    import bench
    p = [0.1, 0.1, 0.1, 1., 1., 7.]
    if tier == 'high':                       # 8.5 - 12 Hz and 30 - 60 Hz from a start at 8: u2 >= 6.5 at every chunk's start
        from oracle import np_models as om_
        p = [0.1, 0.5, 0.1, 0.3, 3., float(om_.g_inv(8.0))]
        ys = np.stack([_sweep(8.5, 12.0, 1800, 1, periods=2.5), _sweep(30.0, 60.0, 1800, 2, periods=2.5)])
        return p, 0.05, ys, lambda rg, n: rg['high'] > 0.5 * n and rg['checked'] == 0
    if tier == 'common':                     # 3.5 - 4.5 Hz from a start at 3.5: never in HIGH, never below 1.5
        p[5] = 3.5
        ys = bench.chirp_batch(4, 3000, 11, Xi=0.1, offset=3.5, meow=100.0)
        return p, 0.1, ys, lambda rg, n: rg['common'] > 0.5 * n and rg['high'] == 0 and rg['checked'] == 0
    if tier == 'low':                        # a negative start the filter does not recover from: u2 <= -1.75
        p[5] = -3.0
        ys = bench.chirp_batch(4, 3000, 5, Xi=0.1, offset=2.0)
        return p, 0.1, ys, lambda rg, n: rg['low'] > 0.5 * n and rg['checked'] == 0
    # 'mid': a start at 0.5 on a 1 - 2 Hz chirp, |u2| < 1.5 at first, then wherever the state goes: the filter leaves the band within a few
    # hundred steps whatever the record, so the bar is that SOME chunks ran there (5 %), not most
    if tier == 'mid':
        p[5] = 0.5
        ys = bench.chirp_batch(4, 3000, 5, Xi=0.1, offset=1.0)
        return p, 0.1, ys, lambda rg, n: rg['mid'] > 0.05 * n and rg['checked'] == 0
    # 'any': a 20 Hz chirp against a start at 7, the state wanders through every band.  The kernel counts no ANY chunks of its own (a chunk
    # that leaves its tier is repeated on the ANY polynomials and counted as `redone`, or goes to the wide step), so `redone + wide > 0` is
    # the nearest evidence the counters give that the ANY step's per-lane angle scale ran; the 1e-9 gate on those records is the check.
    if tier == 'any':
        ys = bench.chirp_batch(4, 3000, 5, Xi=0.1, offset=20.0)
        return p, 0.1, ys, lambda rg, n: rg['wide'] + rg['redone'] > 0 and rg['checked'] == 0
    if tier == 'wide':                       # a wide frequency prior: increments of the angle beyond the bound, those chunks on the wide step
        p[4] = 3.0
        c = cs.chirp_case(T=2000, seed=77)
        ys = c.ys[None, :] + 0.05 * np.random.default_rng(5).standard_normal((8, c.ys.size))
        return p, c.Xi, ys, lambda rg, n: rg['redone'] >= 3 and rg['checked'] == 0
    assert tier == 'checked'                 # a start beyond 700: exp overflows in the reference's naive softplus, NaN in the same places
    p[5] = 705.0
    ys = bench.chirp_batch(4, 1500, 5, Xi=0.1, offset=8.0)
    return p, 0.1, ys, lambda rg, n: rg['checked'] > 0


@pytest.mark.parametrize('tier', ['high', 'common', 'low', 'mid', 'any', 'wide', 'checked'])
def test_records_that_sit_in_each_tier(tier):
    from chirpgp_amd import filters_smoothers as fs, models as pm
    from oracle import port
    p, Xi, ys, shown = _tier_records(tier)
    _, _, disc, m0, P0, H = pm.build_chirp_model(np.array(p))
    want = port.filter(port.F_EKF, disc, None, H, Xi, m0, P0, 1e-3, ys)
    got, rg = _counted(lambda: fs.ekf(disc, H, Xi, m0, P0, 1e-3, ys, **WAVE))
    chunks = ys.shape[0] * ((ys.shape[1] + 63) // 64)
    print(tier, rg)
    assert rg['high'] + rg['common'] + rg['low'] + rg['mid'] + rg['redone'] + rg['wide'] + rg['checked'] == chunks
    assert shown(rg, chunks), (tier, rg, chunks)
    _check(got, want, tier)
    # the four-trials-per-wavefront kernel on the same records (its own tiers: the common-regime step, else the per-lane checked step)
    _check(fs.ekf(disc, H, Xi, m0, P0, 1e-3, ys, **WAVE_X4), want, tier + ' x4')


@pytest.mark.parametrize('kw', [pytest.param(WAVE, id='one_trial_per_wave'), pytest.param(WAVE_X4, id='four_trials_per_wave')])
def test_rising_and_falling_frequency_across_the_tiers(kw):
    """Ramps 2 -> 14 Hz and 14 -> 2 Hz and sweeps that re-cross the bands, from a start at 2 Hz: chunks in MID, COMMON and HIGH, chunks that
    leave their tier and are repeated, and -- in the rotation block's two columns, whose pairs turn in opposite directions -- increments
    of both signs on the way up and on the way down."""
    from chirpgp_amd import filters_smoothers as fs, models as pm
    from oracle import port, np_models as om_
    T, dt, Xi = 3000, 1e-3, 0.05
    ys = np.stack([_ramp(2.0, 14.0, T, 1), _ramp(14.0, 2.0, T, 2), _sweep(2.0, 14.0, T, 3), _sweep(9.0, 3.0, T, 4), _sweep(1.0, 2.0, T, 5)])
    _, _, disc, m0, P0, H = pm.build_chirp_model(np.array([0.1, 0.5, 0.1, 0.3, 3., float(om_.g_inv(2.0))]))
    want = port.filter(port.F_EKF, disc, None, H, Xi, m0, P0, dt, ys)
    u2 = want[0][:, :, 2]
    d = np.diff(np.log1p(np.exp(u2)), axis=1)                              # the angle increments, up to the scale dt 2 pi
    assert ((d > 0).sum(axis=1) > 0.1 * T).all() and ((d < 0).sum(axis=1) > 0.1 * T).all()
    assert u2[0, -500:].mean() > u2[0, 200:700].mean() + 1.0 and u2[1, -500:].mean() < u2[1, 200:700].mean() - 1.0      # rising, falling
    assert (u2[0] < 1.5).any() and (u2[0] > 6.5).any() and (u2[1] > 6.5).any() and (u2[1] < 5.0).any()
    got, rg = _counted(lambda: fs.ekf(disc, H, Xi, m0, P0, dt, ys, **kw))
    print(rg)
    if kw is WAVE:
        assert rg['high'] > 0 and rg['common'] > 0 and rg['mid'] + rg['wide'] > 0 and rg['redone'] > 0, rg
    _check(got, want, 'ramps and sweeps')


@pytest.mark.parametrize('kw', [pytest.param(WAVE, id='one_trial_per_wave'), pytest.param(WAVE_X4, id='four_trials_per_wave')])
def test_lambda_zero_and_la_scala(kw):
    """lambda = 0 (rho = 1: the rotation block undamped) and the La Scala model (no damping parameter at all, its own M32 block)."""
    from chirpgp_amd import filters_smoothers as fs
    from oracle import port
    for c, label in ((cs.chirp_case(T=1500, seed=31, params=(0., 0.3, 0.2, 0.5, 2., 6.)), 'lam0'), (cs.lascala_case(T=1500, seed=32), 'lascala')):
        ys = c.ys[None, :] + 0.05 * np.random.default_rng(9).standard_normal((5, c.ys.size))
        want = port.filter(port.F_EKF, c.disc, None, c.H, c.Xi, c.m0, c.P0, c.dt, ys)
        _check(fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, ys, **kw), want, label)


def test_per_trial_parameters_through_the_four_trial_kernel_and_nll_only():
    """Per-trial model parameters, m0 and P0 (each MFMA block of the x4 kernel carries its own constants and its own column pairs), a
    batch that does not fill its last wavefront; then the NLL-only launch of both kernels (which stays on the common-regime polynomials)."""
    from chirpgp_amd import filters_smoothers as fs, models as pm
    from oracle import port
    B, T = 9, 1000
    rng = np.random.default_rng(3)
    params = np.array([0.1, 0.1, 0.1, 1., 1., 7.]) * rng.uniform(0.7, 1.3, size=(B, 6))
    _, _, disc, m0, P0, H = pm.build_chirp_model(params)
    ys = np.stack([cs.chirp_measurements(T, 200 + i)[2] for i in range(B)])
    want = port.filter(port.F_EKF, disc, None, H, 0.1, m0, P0, 1e-3, ys)
    for kw, label in ((WAVE_X4, 'x4'), (WAVE, 'x1')):
        _check(fs.ekf(disc, H, 0.1, m0, P0, 1e-3, ys, **kw), want, 'per-trial parameters ' + label)
        last = fs.ekf(disc, H, 0.1, m0, P0, 1e-3, ys, nll_final_only=True, want=(False, False, True), **kw)
        assert last[0] is None and last[1] is None
        err = cs.max_rel_err(last[2], want[2][:, -1])
        print('nll only', label, f'{err:.1e}')
        assert err <= GATE, (label, err)


def test_time_split_launch():
    """Four segments with 3008 steps of burn-in: the junction state the kernel records is the mean BY COLUMN and the covariance, as
    before -- the reported mismatch is finite, positive and small, every output within 5 x of it of the sequential launch, the first
    segment IS the sequential launch, and the sequential launch is within the gate of the C port.  (The junction state itself stays on
    the device and has no Python accessor; what this reads of it is the mismatch the kernel computes from it and the segments that start
    from it.)"""
    from chirpgp_amd import filters_smoothers as fs
    from oracle import port
    T, B = 5500, 4
    c = cs.chirp_case(T=3000, seed=90)
    ys = np.tile(c.ys, 2)[None, :T] + 0.05 * np.random.default_rng(7).standard_normal((B, T))
    want = port.filter(port.F_EKF, c.disc, None, c.H, c.Xi, c.m0, c.P0, c.dt, ys)
    seq = fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, ys)
    _check(seq, want, 'sequential')
    got = fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, ys, time_split=(4, 3008), return_junction_error=True)
    err = np.asarray(got[3].cpu()) if hasattr(got[3], 'cpu') else np.asarray(got[3])
    assert err.shape == (B,) and np.isfinite(err).all() and 0 < err.max() < 1e-4, err
    for g, s, w, n in zip(got[:3], seq, want, NAMES):
        assert np.isfinite(g).all()
        rel = float(np.max(np.abs(g - s)) / np.max(np.abs(s)))
        print('time split', n, f'{rel:.1e}', 'junction', f'{err.max():.1e}')
        assert rel <= 5 * err.max() + 1e-14, (n, rel, err)
        assert cs.max_rel_err(g, w) <= max(GATE, 5 * err.max()), n
    assert np.array_equal(got[0][:, :1408], seq[0][:, :1408])


@pytest.mark.parametrize('kw', [pytest.param(WAVE, id='one_trial_per_wave'), pytest.param(WAVE_X4, id='four_trials_per_wave')])
def test_other_measurement_vectors_keep_the_general_form(kw):
    """A measurement vector per trial -- e_1 in some, dense or nearly e_1 in others, so that the four-trial kernel sees mixed wavefronts:
    the general form (eight matrix instructions, the mean in both layouts) is what those run on, and it matches as before."""
    from chirpgp_amd import filters_smoothers as fs
    from oracle import port
    B, T = 9, 600
    c = cs.chirp_case(T=T, seed=41)
    ys = c.ys[None, :] + 0.05 * np.random.default_rng(8).standard_normal((B, T))
    rng = np.random.default_rng(77)
    H = np.tile(np.array([0., 1., 0., 0.]), (B, 1))
    H[[1, 2, 6]] = np.array([0.3, 1., -0.2, 0.1]) + 0.05 * rng.standard_normal((3, 4))
    H[8] = np.array([0., 1., 0., 1e-3])
    want = port.filter(port.F_EKF, c.disc, None, H, c.Xi, c.m0, c.P0, c.dt, ys)
    _check(fs.ekf(c.disc, H, c.Xi, c.m0, c.P0, c.dt, ys, **kw), want, 'per-trial H')
