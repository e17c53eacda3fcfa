"""Randomised records through the regime state machine of the d = 4 EKF kernels.

The headline filter (cgp_mfma4.hpp: ekf4_mfma_kernel) runs 64-step chunks speculatively on lean polynomials chosen by the frequency
state's range -- HIGH (>= 5), common (>= 1.5), LOW (<= -1.5), MID (|x| < 2), the branch-free WIDE step, the checked step -- and repeats a
chunk that left its regime; five counters and thresholds tuned on 45 benchmark sets decide what is tried next.  Hand-built crossing
records test it in test_gpu_parity.py; here 240 seeded random record sets do: frequency-state tracks anywhere in -2 .. 40 (0.1 to 40 Hz)
that cross the boundaries at random places and rates, measurement noise 1e-3 .. 3, dt 1e-3 or 1e-2, T 65 .. 3000, per-trial model
parameters and noise levels, NaN and inf measurements -- through the one-trial-per-wavefront kernel, the four-trials-per-wavefront
kernel and the one-lane-per-trial kernel, each against the C port, NaN and inf positions identical, and the regime counters of the
one-trial kernel accounting for every chunk.

Tolerance, per output array and state component: 1e-9 -- or, for a record set on which the recursion itself is ill-conditioned, 300 x the
amount by which the PORT's own results move when every measurement is perturbed by 1e-15 of itself (measured per set, two runs of the
port); the matrix-core kernels may also use their speculative tiers' designed 1e-11 times that conditioning, up to 1e-7.  Of the 240 sets 228 sit below
1e-10 on all three kernels; the worst (seed 29: dt = 1e-2, the filter 25 units of frequency state away from the signal) moves the port by
1.8e-4 under that perturbation and the kernels by 2.3e-4 .. 5.9e-4 -- the full-accuracy lane kernel as much as the lean-polynomial ones:
it is the recursion that amplifies, not the tiers (ratios to the port's own response: <= 150 over the whole fuzz).

Such a gate has no ceiling, so the second half of the file runs every filter family again RESTARTED from the port's own rows every 64 or 128
steps (tests/fuzz_restart.py): there the amplification is bounded by the segment's length, and every gate has a fixed ceiling that is
asserted on the port's numbers.  The whole-record tests assert how many of their sets the port gates above 1e-9 and above 1e-5."""
import math
from collections import namedtuple

import numpy as np
import pytest

from tests import cases as cs

pytestmark = pytest.mark.gpu

ONE, FOUR, LANE = 0x2 | 0x400, 0x2 | 0x200, 0x4
N_SETS = 240


def _softplus(v):
    return np.logaddexp(0.0, v)


def make_set(seed):
    """One random record set: (B, T, dt, Xi (B,), params (B, 6), ys (B, T), tracks (B, T))."""
    rng = np.random.default_rng(90000 + seed)
    B = int(rng.integers(3, 9))
    T = int(rng.integers(65, 3001))
    dt = 1e-3 if rng.random() < 0.6 else 1e-2
    Xi = 10 ** rng.uniform(-3, math.log10(3.0), size=B)
    if rng.random() < 0.5:
        Xi[:] = Xi[0]
    ts = dt * np.arange(1, T + 1)
    vmax = 40.0 if dt == 1e-3 else 25.0                       # stay well below Nyquist at dt = 1e-2
    params, ys, tracks = np.empty((B, 6)), np.empty((B, T)), np.empty((B, T))
    for b in range(B):
        kind = rng.integers(0, 4)
        if kind == 0:                                         # anywhere to anywhere
            v0, v1 = rng.uniform(-2, vmax, size=2)
        elif kind == 1:                                       # around the common / MID / LOW boundaries
            v0, v1 = rng.uniform(-2.5, 3.0, size=2)
        elif kind == 2:                                       # around the HIGH boundary
            v0, v1 = rng.uniform(3.5, 7.0, size=2)
        else:                                                 # flat
            v0 = rng.uniform(-2, vmax)
            v1 = v0 + rng.uniform(-0.3, 0.3)
        cyc = rng.uniform(0.3, 2.5)
        v = v0 + (v1 - v0) * 0.5 * (1 - np.cos(2 * math.pi * cyc * np.arange(T) / T))
        tracks[b] = v
        phase = np.cumsum(_softplus(v)) * dt
        amp = rng.uniform(0.5, 2.0)
        ys[b] = amp * np.sin(2 * math.pi * phase + rng.uniform(0, 2 * math.pi)) + math.sqrt(Xi[b]) * rng.standard_normal(T)
        params[b] = np.array([0.1, rng.uniform(0.05, 0.6), 0.1, rng.uniform(0.3, 1.2), rng.uniform(0.8, 3.0), v0]) * np.r_[rng.uniform(0.7, 1.3, 5), 1.0]
        if rng.random() < 0.1:
            params[b, 0] = 0.0                                # the lam = 0 branch of models.py:302-308
    if rng.random() < 0.15:
        ys[rng.integers(0, B), rng.integers(0, T)] = np.nan
    if rng.random() < 0.08:
        ys[rng.integers(0, B), rng.integers(0, T)] = np.inf
    return B, T, dt, Xi, params, ys, tracks


def distance(g, w, n):
    """Largest error of an output array, component by component, each against ITS scale: the frequency state runs up to 40, the chirp's
    amplitude is ~1 -- one denominator for the whole vector would hide the small components, and an element-wise floor of 1e-3 of the global
    scale would gate them at 1e-12 of theirs.  Non-finite entries (compared separately) count as 0."""
    bad = ~(np.isfinite(w) & np.isfinite(g))
    gf, wf = np.where(bad, 0.0, g), np.where(bad, 0.0, w)
    if n == 'mfs':
        return max(cs.max_rel_err(gf[..., c], wf[..., c]) for c in range(4))
    if n == 'Pfs':
        sd = np.sqrt(np.maximum(np.abs(wf[..., np.arange(4), np.arange(4)]).reshape(-1, 4).max(axis=0), 1e-300))
        return max(float(np.abs(gf[..., i, j] - wf[..., i, j]).max() / (sd[i] * sd[j])) for i in range(4) for j in range(4))
    return cs.max_rel_err(gf, wf)


# How many sets of each whole-record test may be gated above 1e-9 and above 1e-5: what the PORT alone gives (the gates are functions of the
# port's response to the 1e-15 perturbation, no kernel enters), plus 10 % rounded up.  A set gated above 1e-5 is, in effect, not compared by
# the whole-record test; each such seed is named in its test's docstring, and the restarted tests below cover it under a fixed ceiling.
WHOLE_RECORD_GATES = {           # test: (sets above 1e-9 as measured, allowed, sets above 1e-5 as measured, allowed)
    'ekf': (28, 31, 3, 4),
    'gh3_d4': (41, 46, 0, 0),
    'cubature_d8': (42, 47, 2, 3),
    # the next two tests have one gate, max(1e-9, 300 delta, min(1e-7, 2e4 delta)); like the tests above they count the sets on its
    # max(1e-9, 300 delta) term (the last term lifts all 40 / 36 of 48 sets above 1e-9 and ends at 1e-7: a count on it would assert nothing)
    'smoothers_cd': (27, 30, 0, 0),
    'other_kernels': (10, 11, 0, 0),
}


def _assert_gate_counts(test, gates):
    """gates: {seed: the set's largest whole-record max(1e-9, 300 delta)} (the min(1e-7, 2e4 delta) term never reaches 1e-5).  Prints the seeds above 1e-9 and above 1e-5, asserts their numbers."""
    above9 = sorted(s for s, t in gates.items() if t > 1e-9)
    above5 = sorted((s for s, t in gates.items() if t > 1e-5), key=lambda s: -gates[s])
    print(f'{test}: {len(above9)} of {len(gates)} sets gated above 1e-9 (the port alone decides): seeds {above9}')
    print(f'{test}: {len(above5)} gated above 1e-5: ' + ', '.join(f'seed {s} at {gates[s]:.1e}' for s in above5))
    _, allowed9, _, allowed5 = WHOLE_RECORD_GATES[test]
    assert len(above9) <= allowed9, (test, 'the PORT moved: sets gated above 1e-9', len(above9), allowed9, above9)
    assert len(above5) <= allowed5, (test, 'the PORT moved: sets gated above 1e-5', len(above5), allowed5, above5)


def test_random_records_through_the_regime_state_machine():
    """The whole records (the module's docstring).  Of the 240 sets the port alone gates 28 above 1e-9 and three above 1e-5 -- seed 29 (5.5e-2),
    seed 138 (1.3e-5), seed 199 (1.0e-5): on those this test compares, in effect, nothing; test_ekf_restarted_from_the_ports_rows covers
    them, like every other set, under its fixed ceiling of 1e-8.  The two counts are asserted (WHOLE_RECORD_GATES), the seeds printed."""
    from chirpgp_amd import filters_smoothers as fs, models as pm, _engine
    from oracle import port
    totals = dict.fromkeys(_engine.REGIME_COUNTERS, 0)
    worst = {ONE: 0.0, FOUR: 0.0, LANE: 0.0}
    ill = 0
    failures = []
    below = arrays = 0
    gates = {}
    for seed in range(N_SETS):
        B, T, dt, Xi, params, ys, tracks = make_set(seed)
        drift, disp, disc, m0, P0, H = pm.build_chirp_model(params)
        want = port.filter(port.F_EKF, disc, None, H, Xi, m0, P0, dt, ys)
        # the recursion's own conditioning on this set: how far the port moves when every measurement moves by 1e-15 of itself
        moved = port.filter(port.F_EKF, disc, None, H, Xi, m0, P0, dt, ys * (1 + 1e-15 * np.random.default_rng(seed).choice([-1., 1.], size=ys.shape)))
        delta = {n: distance(np.asarray(b_), np.asarray(a), n) for a, b_, n in zip(want, moved, ('mfs', 'Pfs', 'nll'))}
        # kappa = delta / 1e-15 is the set's conditioning.  The lane kernel evaluates every function to a few ulp: 300 delta covers it (<= 150
        # seen).  The speculative tiers of the matrix-core kernels inject 1e-11 (LOW: 1.6e-9) by design (cgp_mfma4.hpp) -- kappa x 2e-11 is
        # theirs to use, but never more than 1e-7 on that account (seen: 7.5e-9 at kappa = 1.7e4, seed 23)
        tols = {n: max(1e-9, 300.0 * d) for n, d in delta.items()}
        tols_lean = {n: max(tols[n], min(1e-7, 2e4 * d)) for n, d in delta.items()}
        ill += max(tols.values()) > 1e-9
        gates[seed] = max(tols.values())
        for flags in (ONE, FOUR, LANE):
            if flags == ONE:
                _engine.debug_set(_engine.DBG_COUNT_REGIMES, 1)
                _engine.debug_counters(reset=True)
            got = fs.ekf(disc, H, Xi, m0, P0, dt, ys, flags=flags)
            if flags == ONE:
                rg = _engine.debug_counters(reset=True)
                _engine.debug_set(_engine.DBG_COUNT_REGIMES, 0)
                chunks = B * ((T + 63) // 64)
                kept = rg['high'] + rg['common'] + rg['low'] + rg['mid'] + rg['redone'] + rg['wide'] + rg['checked']
                if kept != chunks:
                    failures.append((seed, 'counters', kept, chunks, rg))
                for k in totals:
                    totals[k] += rg[k]
            for g, w, n in zip(got, want, ('mfs', 'Pfs', 'nll')):
                g, w = np.asarray(g), np.asarray(w)
                # non-finite entries (an inf measurement gives inf, then NaN) must be the SAME non-finite values; the rest is compared
                bad = ~np.isfinite(w)
                if not (np.array_equal(bad, ~np.isfinite(g)) and np.array_equal(np.isnan(w), np.isnan(g)) and np.array_equal(np.sign(w[bad & ~np.isnan(w)]), np.sign(g[bad & ~np.isnan(w)]))):
                    failures.append((seed, flags, n, 'non-finite entries differ', dict(B=B, T=T, dt=dt)))
                    continue
                e, tol = distance(g, w, n), (tols if flags == LANE else tols_lean)[n]
                if not e <= tol:
                    failures.append((seed, flags, n, f'{e:.3e} > {tol:.1e}', dict(B=B, T=T, dt=dt, delta=delta[n])))
                worst[flags] = max(worst[flags], e)
                below += e < 1e-10
                arrays += 1
                if e > 1e-9:
                    print(f'  seed {seed} flags {flags:#x} {n}: {e:.2e}  (B {B} T {T} dt {dt}; the port under a 1e-15 perturbation: {delta[n]:.2e})')
    print(f'{N_SETS} sets ({ill} ill-conditioned: tolerance above 1e-9); {below} of {arrays} output arrays below 1e-10; worst relative error one-trial {worst[ONE]:.2e}, four-trials {worst[FOUR]:.2e}, lane {worst[LANE]:.2e}')
    print('chunks by regime over the fuzz:', totals)
    _assert_gate_counts('ekf', gates)
    assert not failures, failures[:6]
    # the fuzz reached every tier of the state machine
    for k in ('high', 'common', 'low', 'mid', 'wide', 'redone'):
        assert totals[k] > 0, (k, totals)


# ------------------------------------------------------------------------------------------------ the sigma-point filters' tiers
def _dist_any(g, w, n, d):
    bad = ~(np.isfinite(w) & np.isfinite(g))
    gf, wf = np.where(bad, 0.0, g), np.where(bad, 0.0, w)
    if n == 'mfs':
        return max(cs.max_rel_err(gf[..., c], wf[..., c]) for c in range(d))
    if n == 'Pfs':
        sd = np.sqrt(np.maximum(np.abs(wf[..., np.arange(d), np.arange(d)]).reshape(-1, d).max(axis=0), 1e-300))
        return max(float(np.abs(gf[..., i, j] - wf[..., i, j]).max() / (sd[i] * sd[j])) for i in range(d) for j in range(d))
    return cs.max_rel_err(gf, wf)


@pytest.mark.parametrize('config', ['gh3_d4', 'cubature_d8'])
def test_random_records_through_the_sigma_point_filters(config):
    """The sigma-point filters speculate too (cgp_mfma4_sigma.hpp, cgp_coop8.hpp, cgp_lane4.hpp: a lean fan where every point's frequency state
    sits in the common regime, a branch-free full-accuracy fan behind it, the checked fan beyond 700): the same random record sets -- tracks
    that cross the bands anywhere, per-trial parameters and noise levels, NaN / inf measurements -- through sgp_filter with Gauss-Hermite order 3
    on the d = 4 chirp model (one wavefront per trial AND one lane per trial) and with the cubature rule on the three-harmonic model (d = 8, tile
    layout), against the C port under the conditioning-based gate of the EKF fuzz.

    Whole-record gates as the port alone gives them: GH-3 41 of 60 sets above 1e-9, none above 1e-5 (largest 8.5e-8); cubature 42 above 1e-9 and
    two above 1e-5 -- seed 1036 (gate 3.2e2: the port's means move by O(1)) and seed 1056 (9.3e-2), on which this test compares nothing;
    test_sigma_point_filters_restarted_from_the_ports_rows covers them under its ceiling of 1e-6.  Counts asserted (WHOLE_RECORD_GATES), seeds printed."""
    from chirpgp_amd import filters_smoothers as fs, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    from oracle import port
    d = 4 if config == 'gh3_d4' else 8
    sgps = SigmaPoints.gauss_hermite(4, 3) if config == 'gh3_d4' else SigmaPoints.cubature(8)
    shapes = ((0x2, 'wave'), (0x4, 'lane')) if config == 'gh3_d4' else ((0x2, 'wave'),)
    failures, worst, ill, below, arrays = [], dict.fromkeys([s for _, s in shapes], 0.0), 0, 0, 0
    gates = {}
    n_sets = 60
    for seed in range(n_sets):
        B, T, dt, Xi, params, ys, _ = make_set(1000 + seed)
        T = min(T, 1200)
        ys = np.ascontiguousarray(ys[:, :T])
        if config == 'gh3_d4':
            _, _, disc, m0, P0, H = pm.build_chirp_model(params)
        else:
            _, _, disc, m0, P0, H = pm.build_harmonic_chirp_model(params, num_harmonics=3)
        want = port.filter(port.F_SGP, disc, sgps, H, Xi, m0, P0, dt, ys)
        moved = port.filter(port.F_SGP, disc, sgps, H, Xi, m0, P0, dt, ys * (1 + 1e-15 * np.random.default_rng(seed).choice([-1., 1.], size=ys.shape)))
        delta = {n: _dist_any(np.asarray(b_), np.asarray(a), n, d) for a, b_, n in zip(want, moved, ('mfs', 'Pfs', 'nll'))}
        tols = {n: max(1e-9, 300.0 * v) for n, v in delta.items()}
        tols_lean = {n: max(tols[n], min(1e-7, 2e4 * v)) for n, v in delta.items()}
        ill += max(tols.values()) > 1e-9
        gates[1000 + seed] = max(tols.values())
        for flags, shape in shapes:
            got = fs.sgp_filter(disc, sgps, H, Xi, m0, P0, dt, ys, flags=flags)
            for g, w, n in zip(got, want, ('mfs', 'Pfs', 'nll')):
                g, w = np.asarray(g), np.asarray(w)
                bad = ~np.isfinite(w)
                if not (np.array_equal(bad, ~np.isfinite(g)) and np.array_equal(np.isnan(w), np.isnan(g))):
                    failures.append((seed, shape, n, 'non-finite entries differ', dict(B=B, T=T, dt=dt)))
                    continue
                e, tol = _dist_any(g, w, n, d), tols_lean[n]
                if not e <= tol:
                    failures.append((seed, shape, n, f'{e:.3e} > {tol:.1e}', dict(B=B, T=T, dt=dt, delta=delta[n])))
                worst[shape] = max(worst[shape], e)
                below += e < 1e-10
                arrays += 1
                if e > 1e-9:
                    print(f'  seed {seed} {shape} {n}: {e:.2e}  (B {B} T {T} dt {dt}; the port under a 1e-15 perturbation: {delta[n]:.2e})')
    print(f'{config}: {n_sets} sets ({ill} ill-conditioned); {below} of {arrays} output arrays below 1e-10; worst ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    _assert_gate_counts(config, gates)
    assert not failures, failures[:6]


def _broken_from(want):
    """Per trial, the first step at which the port's filter has broken down -- a negative variance or a NaN likelihood (RK4 at dt = 1e-2 on a 20 Hz
    chirp loses the covariance's definiteness; the reference returns NaN from there on).  What any float64 implementation computes behind that
    point is the rounding noise of differences of 1e80-sized numbers: the port's own sample of it is reproduced only by a kernel with the port's
    operation order (the DPP kernels do, to 1e-10; the matrix-core ones do not), and nothing is compared there."""
    Pd = np.asarray(want[1])[..., np.arange(4), np.arange(4)]
    ok = np.isfinite(np.asarray(want[2])) & (Pd > 0).all(axis=-1) & np.isfinite(np.asarray(want[0])).all(axis=-1)
    return np.where(ok.all(axis=1), ok.shape[1], np.argmin(ok, axis=1))


def test_random_records_through_the_smoothers_and_the_continuous_discrete_filters():
    """The rest of the d = 4 chirp kernels on the random record sets: eks and cd_eks in both launch shapes (the walk / the matrix-core kernel, and one
    lane per trial), sgp_smoother and cd_sgp_smoother (Gauss-Hermite order 3) on the port's filtering rows, cd_ekf and cd_sgp_filter on the
    records -- each against the C port under the conditioning-based gate (the smoothers are run on IDENTICAL filtering rows, so their gate is the
    plain 1e-9 unless the port's smoother itself moves under a 1e-15 perturbation of those rows).

    Whole-record gates as the port alone gives them: 27 of the 40 sets have a max(1e-9, 300 delta) above 1e-9 (with the min(1e-7, 2e4 delta) term
    every one of the 40: sgp_smoother's) and none a gate above 1e-7, so none above 1e-5: no smoother set is left uncompared, which matters
    because a smoother starts from the last filtering row and has no restarted form.  The filters' restarted form is
    test_continuous_discrete_filters_restarted_from_the_ports_rows.  Counts asserted (WHOLE_RECORD_GATES), seeds printed."""
    import copy
    from chirpgp_amd import filters_smoothers as fs, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    from oracle import port
    gh3 = SigmaPoints.gauss_hermite(4, 3)
    failures, worst, arrays, below, broken, overflowed = [], {}, 0, 0, 0, 0
    gates = {}
    broken_from = _broken_from

    def check(tag, seed, got, want, moved, info, until=None, valid=None):
        nonlocal arrays, below
        for i, (g, w, mv) in enumerate(zip(got, want, moved)):
            g, w, mv = np.array(g), np.array(w), np.array(mv)
            if until is not None:
                for b, t in enumerate(until):
                    g[b, t:], w[b, t:], mv[b, t:] = 0.0, 0.0, 0.0
            if valid is not None:
                g[~valid], w[~valid], mv[~valid] = 0.0, 0.0, 0.0
            n = ('mfs', 'Pfs', 'nll')[i]
            bad = ~np.isfinite(w)
            if not (np.array_equal(bad, ~np.isfinite(g)) and np.array_equal(np.isnan(w), np.isnan(g))):
                failures.append((seed, tag, n, 'non-finite entries differ', info))
                continue
            delta = _dist_any(mv, w, n, 4)
            tol = max(1e-9, 300.0 * delta, min(1e-7, 2e4 * delta))
            gates[2000 + seed] = max(gates.get(2000 + seed, 0.0), 1e-9, 300.0 * delta)
            e = _dist_any(g, w, n, 4)
            if not e <= tol:
                failures.append((seed, tag, n, f'{e:.3e} > {tol:.1e}', dict(info, delta=delta)))
            worst[tag] = max(worst.get(tag, 0.0), e)
            arrays += 1
            below += e < 1e-10

    for seed in range(40):
        B, T, dt, Xi, params, ys, _ = make_set(2000 + seed)
        T = min(T, 800)
        ys = np.ascontiguousarray(ys[:, :T])
        info = dict(B=B, T=T, dt=dt)
        drift, disp, disc, m0, P0, H = pm.build_chirp_model(params)
        dg = copy.copy(drift)
        dg.gamma = disp.outer()
        sign = np.random.default_rng(seed).choice([-1., 1.], size=ys.shape)
        ys_moved = ys * (1 + 1e-15 * sign)
        # ---- continuous-discrete filters on the records
        for tag, method, sg, run in (('cd_ekf', port.F_CD_EKF, None, lambda: fs.cd_ekf(drift, disp, H, Xi, m0, P0, dt, ys)),
                                     ('cd_sgp_filter', port.F_CD_SGP, gh3, lambda: fs.cd_sgp_filter(drift, disp(None), gh3, H, Xi, m0, P0, dt, ys))):
            want = port.filter(method, dg, sg, H, Xi, m0, P0, dt, ys)
            moved = port.filter(method, dg, sg, H, Xi, m0, P0, dt, ys_moved)
            until = broken_from(want)
            broken += int((until < T).sum())
            check(tag, seed, run(), want, moved, info, until)
        # ---- smoothers on the port's filtering rows (finite records only: a NaN row makes every earlier smoothed row NaN, nothing to compare)
        fd = port.filter(port.F_EKF, disc, None, H, Xi, m0, P0, dt, ys)
        fc = port.filter(port.F_CD_EKF, dg, None, H, Xi, m0, P0, dt, ys)
        # (filtering rows a smoother can be asked to smooth: finite and positive definite throughout, from either filter)
        finite = np.isfinite(ys).all(axis=1) & (broken_from(fd) == T) & (broken_from(fc) == T)
        if not finite.any():
            continue
        sel = np.flatnonzero(finite)
        prm = params[sel]
        drift_s, disp_s, disc_s, _, _, _ = pm.build_chirp_model(prm)
        dg_s = copy.copy(drift_s)
        dg_s.gamma = disp_s.outer()
        for tag, method, model, sg, f, runs in (
                ('eks', port.S_EKS, disc_s, None, fd, {'wave': lambda m, P: fs.eks(disc_s, m, P, dt, flags=0x2), 'lane': lambda m, P: fs.eks(disc_s, m, P, dt, flags=0x4)}),
                ('sgp_smoother', port.S_SGP, disc_s, gh3, fd, {'wave': lambda m, P: fs.sgp_smoother(disc_s, gh3, m, P, dt, flags=0x2)}),
                ('cd_eks', port.S_CD_EKS, dg_s, None, fc, {'wave': lambda m, P: fs.cd_eks(drift_s, disp_s, m, P, dt, flags=0x2), 'lane': lambda m, P: fs.cd_eks(drift_s, disp_s, m, P, dt, flags=0x4)}),
                ('cd_sgp_smoother', port.S_CD_SGP, dg_s, gh3, fc, {'wave': lambda m, P: fs.cd_sgp_smoother(drift_s, disp_s(None), gh3, m, P, dt, flags=0x2)})):
            m, P = np.ascontiguousarray(f[0][sel]), np.ascontiguousarray(f[1][sel])
            if not (np.isfinite(m).all() and np.isfinite(P).all()):
                continue
            want = port.smoother(method, model, sg, dt, m, P)
            moved = port.smoother(method, model, sg, dt, m * (1 + 1e-15), P)
            # the backward RK4 can overflow as well (dt = 1e-2): rows are compared from the end of the record down to the port's first non-finite
            # one; behind it the implementations differ in where inf turns into NaN, which is nobody's result
            ok = np.isfinite(want[0]).all(axis=-1) & np.isfinite(want[1]).all(axis=(-1, -2))
            valid = np.flip(np.logical_and.accumulate(np.flip(ok, axis=1), axis=1), axis=1)
            overflowed += int((~valid.all(axis=1)).sum())
            for shape, run in runs.items():
                check(f'{tag} {shape}', seed, run(m, P), want, moved, info, valid=valid)
    print(f'{broken} (trial, filter) pairs broke down and {overflowed} (trial, smoother) pairs overflowed (compared up to there); {below} of {arrays} output arrays below 1e-10; worst by kernel: ' + ', '.join(f'{k} {v:.1e}' for k, v in sorted(worst.items())))
    _assert_gate_counts('smoothers_cd', gates)
    assert not failures, failures[:6]


def _gate(g, w, mv, n, d):
    """(error, tolerance, the tolerance's max(1e-9, 300 delta) term) of one output array under the fuzz's conditioning-based gate; None if the
    non-finite patterns differ."""
    g, w, mv = np.asarray(g), np.asarray(w), np.asarray(mv)
    bad = ~np.isfinite(w)
    if not (np.array_equal(bad, ~np.isfinite(g)) and np.array_equal(np.isnan(w), np.isnan(g))):
        return None
    delta = _dist_any(mv, w, n, d)
    return _dist_any(g, w, n, d), max(1e-9, 300.0 * delta, min(1e-7, 2e4 * delta)), max(1e-9, 300.0 * delta)


def _random_model_set(seed):
    """One set of test_random_models_through_the_other_kernels -> (B, T, signs of the perturbation, the linear model (d, F, Sigma, H, Xi, m0, P0, ys),
    dt, the toy chirp records, kind, the kind's own draws): kind 0 = La Scala parameters (B, 4); 1 = (harmonics, harmonic-model parameters (B, 6));
    2 = (harmonics, KPT case, its records (B, T))."""
    rng = np.random.default_rng(70000 + seed)
    B, T = int(rng.integers(2, 7)), int(rng.integers(30, 700))
    sign = rng.choice([-1., 1.], size=(B, T))
    d = 1 + seed % 8
    A = rng.standard_normal((d, d))
    F = 0.97 * A / max(np.abs(np.linalg.eigvals(A)).max(), 1e-3) if d > 1 else np.array([[0.9]])
    L = 0.3 * rng.standard_normal((d, d))
    Sigma = L @ L.T + 0.01 * np.eye(d)
    H = rng.standard_normal(d)
    Xi = 10 ** rng.uniform(-2, 0)
    m0, P0 = rng.standard_normal(d), np.eye(d) * rng.uniform(0.2, 2.0)
    ys = rng.standard_normal((B, T))
    if rng.random() < 0.3:
        ys[rng.integers(0, B), rng.integers(0, T)] = np.nan
    dt = 1e-3
    ts = dt * np.arange(1, T + 1)
    f0 = rng.uniform(2.0, 12.0, size=(B, 1))
    ysc = np.sin(2 * np.pi * (f0 * ts + 0.5 * rng.uniform(-3, 3, size=(B, 1)) * ts ** 2)) + np.sqrt(0.1) * rng.standard_normal((B, T))
    kind = seed % 3
    if kind == 0:
        toy = np.array([0.1, 1.0, 1.0, 7.0]) * rng.uniform(0.6, 1.5, size=(B, 4))
    elif kind == 1:
        toy = 2 + (seed // 3) % 2, np.array([0.1, 0.1, 0.1, 1.0, 1.0, 7.0]) * rng.uniform(0.6, 1.5, size=(B, 6))
    else:
        nh = 1 + (seed // 3) % 3
        c = cs.kpt_case(T=max(T, 2), seed=seed, nh=nh, params=tuple(np.array([0.5, 1e-4, 0.1, 8., 1.]) * rng.uniform(0.7, 1.4, size=5)))
        toy = nh, c, c.ys[None, :T] + 0.05 * rng.standard_normal((B, T))
    return B, T, sign, (d, F, Sigma, H, Xi, m0, P0, ys), dt, ysc, kind, toy


def test_random_models_through_the_other_kernels():
    """What the chirp fuzz does not reach: the linear kernels at every dimension 1 .. 8 (kf + rts on random stable F, Sigma: generic, d = 4 matrix-core /
    walk and d >= 5 tile-layout kernels, whole-record and time-split smoothers), the La Scala model (ekf, eks, sgp_filter: the chirp kernels on
    its parameter layout), the harmonic models at d = 6 and 8 (ekf + eks in the tile layout and per lane), and ekf_for_kpt at d = 3, 4, 5 -- random
    parameters, noise levels, record lengths and NaN measurements, against the C port under the conditioning-based gate.

    Whole-record gates as the port alone gives them: 10 of the 48 sets have a max(1e-9, 300 delta) above 1e-9 (36 with the min(1e-7, 2e4 delta) term:
    La Scala sgp_filter and eks, the harmonic eks and the three-harmonic ekf, KPT; the linear kernels never), the largest 3e-6 (KPT with three
    harmonics, seed 8), none above 1e-5.  The filters among them are run
    again in test_other_models_restarted_from_the_ports_rows; the smoothers (largest gate 3e-9) have no restarted form and need none.  Counts
    asserted (WHOLE_RECORD_GATES), seeds printed."""
    from chirpgp_amd import filters_smoothers as fs, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    from oracle import port
    failures, worst, arrays, below = [], {}, 0, 0
    gates = {}

    def compare(tag, seed, got, want, moved, d, names=('mfs', 'Pfs', 'nll')):
        nonlocal arrays, below
        for g, w, mv, n in zip(got, want, moved, names):
            r = _gate(g, w, mv, n, d)
            if r is None:
                failures.append((seed, tag, n, 'non-finite entries differ'))
                continue
            e, tol, tol300 = r
            gates[seed] = max(gates.get(seed, 0.0), tol300)
            if not e <= tol:
                failures.append((seed, tag, n, f'{e:.3e} > {tol:.1e}'))
            worst[tag] = max(worst.get(tag, 0.0), e)
            arrays += 1
            below += e < 1e-10

    for seed in range(48):
        B, T, sign, (d, F, Sigma, H, Xi, m0, P0, ys), dt, ysc, kind, toy = _random_model_set(seed)
        # ---- linear: kf + rts, d = 1 .. 8
        lin = pm.linear_cond_m_cov(F, Sigma)
        want = port.filter(port.F_EKF, lin, None, H, Xi, m0, P0, 0.0, ys)
        moved = port.filter(port.F_EKF, lin, None, H, Xi, m0, P0, 0.0, ys * (1 + 1e-15 * sign))
        for name, fl in (('wave', 0x2), ('lane', 0x4), ('generic', 0x12)):
            compare(f'kf d{d} {name}', seed, fs.kf(F, Sigma, H, Xi, m0, P0, ys, flags=fl), want, moved, d)
        ok = np.isfinite(ys).all(axis=1)
        if ok.any():
            m, P = np.ascontiguousarray(want[0][ok]), np.ascontiguousarray(want[1][ok])
            ws = port.smoother(port.S_EKS, lin, None, 0.0, m, P)
            ms = port.smoother(port.S_EKS, lin, None, 0.0, m * (1 + 1e-15), P)
            for name, fl in (('wave', 0x2), ('lane', 0x4), ('generic', 0x12), ('time-split', 0x2 | 0x800)):
                compare(f'rts d{d} {name}', seed, fs.rts(F, Sigma, m, P, flags=fl), ws, ms, d, ('mfs', 'Pfs'))
        # ---- La Scala (d = 4), harmonic (d = 6, 8), KPT (d = 3, 4, 5): a toy chirp per trial
        if kind == 0:
            prm = toy
            _, _, disc, m0c, P0c, Hc = pm.build_lascala_model(prm)
            gh3 = SigmaPoints.gauss_hermite(4, 3)
            for tag, method, sg, run in (('lascala ekf', port.F_EKF, None, lambda fl: fs.ekf(disc, Hc, 0.1, m0c, P0c, dt, ysc, flags=fl)),
                                         ('lascala sgp_filter', port.F_SGP, gh3, lambda fl: fs.sgp_filter(disc, gh3, Hc, 0.1, m0c, P0c, dt, ysc, flags=fl))):
                want = port.filter(method, disc, sg, Hc, 0.1, m0c, P0c, dt, ysc)
                moved = port.filter(method, disc, sg, Hc, 0.1, m0c, P0c, dt, ysc * (1 + 1e-15 * sign))
                for name, fl in (('wave', 0x2), ('lane', 0x4)):
                    compare(f'{tag} {name}', seed, run(fl), want, moved, 4)
                if sg is None:
                    ws = port.smoother(port.S_EKS, disc, None, dt, want[0], want[1])
                    ms = port.smoother(port.S_EKS, disc, None, dt, want[0] * (1 + 1e-15), want[1])
                    for name, fl in (('wave', 0x2), ('lane', 0x4), ('time-split', 0x2 | 0x800)):
                        compare(f'lascala eks {name}', seed, fs.eks(disc, want[0], want[1], dt, flags=fl), ws, ms, 4, ('mfs', 'Pfs'))
        elif kind == 1:
            nh, prm = toy
            dd = 2 * nh + 2
            _, _, disc, m0c, P0c, Hc = pm.build_harmonic_chirp_model(prm, num_harmonics=nh)
            want = port.filter(port.F_EKF, disc, None, Hc, 0.1, m0c, P0c, dt, ysc)
            moved = port.filter(port.F_EKF, disc, None, Hc, 0.1, m0c, P0c, dt, ysc * (1 + 1e-15 * sign))
            for name, fl in (('wave', 0x2), ('lane', 0x4)):
                compare(f'harmonic{nh} ekf {name}', seed, fs.ekf(disc, Hc, 0.1, m0c, P0c, dt, ysc, flags=fl), want, moved, dd)
            ws = port.smoother(port.S_EKS, disc, None, dt, want[0], want[1])
            ms = port.smoother(port.S_EKS, disc, None, dt, want[0] * (1 + 1e-15), want[1])
            for name, fl in (('wave', 0x2), ('lane', 0x4), ('time-split', 0x2 | 0x800)):
                compare(f'harmonic{nh} eks {name}', seed, fs.eks(disc, want[0], want[1], dt, flags=fl), ws, ms, dd, ('mfs', 'Pfs'))
        else:
            nh, c, yk = toy
            spec = pm.linear_cond_m_cov(c.F, c.Sigma)
            spec.model_id, spec.n_harm = pm.M_KPT, nh
            want = port.filter(port.F_EKF_KPT, spec, None, None, c.Xi, c.m0, c.P0, c.dt, yk)
            moved = port.filter(port.F_EKF_KPT, spec, None, None, c.Xi, c.m0, c.P0, c.dt, yk * (1 + 1e-15 * sign))
            for name, fl in (('wave', 0x2), ('lane', 0x4), ('generic', 0x12)):
                compare(f'kpt{nh} {name}', seed, fs.ekf_for_kpt(c.F, c.Sigma, c.h, c.Xi, c.m0, c.P0, c.dt, yk, flags=fl), want, moved, nh + 2)
    print(f'{below} of {arrays} output arrays below 1e-10; worst by kernel family: ' +
          ', '.join(f'{k} {v:.1e}' for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:12]))
    _assert_gate_counts('other_kernels', gates)
    assert not failures, failures[:8]


# ------------------------------------------------------------------------------------------------ restarted from the port's rows
# The whole-record gates above follow the recursion's amplification wherever it goes: 5.5e-2 on EKF seed 29, 318 on one d = 8 set.  The
# amplification comes from the LENGTH of the record, so the same sets are run again in segments of L steps, each started from the port's own
# row just before it (tests/fuzz_restart.py): the same states in the same tiers, under a gate that has a fixed ceiling.
def _same_nonfinite(g, w, signs):
    bad = ~np.isfinite(w)
    if not (np.array_equal(bad, ~np.isfinite(g)) and np.array_equal(np.isnan(w), np.isnan(g))):
        return False
    inf = bad & ~np.isnan(w)
    return not signs or np.array_equal(np.sign(w[inf]), np.sign(g[inf]))


# One fuzz set for _run_restarted: info (printed with a failure), the state dimension d, the port's whole-record result want, the set (m0, P0,
# params, Xi, H, ys), the signs of its 1e-15 perturbation, port_on(seg, ys) = the port on a batch of segments with the measurements ys, and
# kernels = {name: (run(seg), lean)}
FuzzSet = namedtuple('FuzzSet', 'info d want m0 P0 params Xi H ys sign port_on kernels')

# Ceilings of test_other_models_restarted_from_the_ports_rows: (on max(1e-9, 300 delta_seg), on the lean gate) -- its docstring
OTHER_CEILINGS = {'lascala': (1e-9, 1e-9), 'lascala sgp_filter': (1e-8, 1e-7), 'harmonic': (1e-9, 1e-8), 'kpt': (1e-5, 1e-5)}


def _run_restarted(family, seeds, L, setup, ceiling, lean_ceiling, drop_cap, until_breakdown=False, signs=False):
    """One family of fuzz sets in restarted form; setup(seed) -> FuzzSet.  Reference: the port ON THE SEGMENTS (a segment's NLL starts at 0).
    delta: the port's response, segment-wise, to the whole-record tests' 1e-15 sign perturbation of the measurements; distances over all
    segments of a set at once, so the scales are the set's.  Gate: max(1e-9, 300 delta); a kernel with speculative tiers (lean) gets
    max(1e-9, 300 delta, min(1e-7, 2e4 delta)).  Asserted on the port's numbers alone: the first gate of every set and array <= ceiling, the
    second <= lean_ceiling, the share of dropped segments <= drop_cap.  Both ceilings follow one rule: the port's largest 300 delta (2e4 delta)
    over the family, the larger of the two hosts' x 3, rounded up to a power of ten, at least the gate's floor of 1e-9 and at most 1e-5 (at
    most max(ceiling, 1e-7) for the lean gate, whose extra term ends at 1e-7)."""
    from tests import fuzz_restart as fr
    names = ('mfs', 'Pfs', 'nll')
    failures, port_moved, worst, gates = [], [], {}, {}
    total = dropped = arrays = below = 0
    raw = (0.0, None)
    for seed in seeds:
        fz = setup(seed)
        info, d, port_on = fz.info, fz.d, fz.port_on
        ys_moved = fz.ys * (1 + 1e-15 * fz.sign)
        batches, n, k = fr.restart_batches(fz.want, fz.m0, fz.P0, fz.params, fz.Xi, fz.H, fz.ys, L)
        total += n
        dropped += k
        wants = [port_on(s, s.ys) for s in batches]
        moveds = [port_on(s, fr.cut(s, ys_moved)) for s in batches]
        untils = [_broken_from(w) if until_breakdown else None for w in wants]
        dropped += sum(int((u == 0).sum()) for u in untils if u is not None)       # broken down at its first step: nothing is compared

        def table(results):
            """The three output arrays of the set's batches as rows over all its segments, nothing behind a breakdown."""
            out = []
            for i in range(3):
                parts = []
                for r, u in zip(results, untils):
                    a = np.array(r[i])
                    if u is not None:
                        for j, t in enumerate(u):
                            a[j, t:] = 0.0
                    parts.append(a)
                out.append(fr.rows(parts, (1, 2, 0)[i]))
            return out

        w3, mv3 = table(wants), table(moveds)
        delta = {n_: _dist_any(mv, w, n_, d) for mv, w, n_ in zip(mv3, w3, names)}
        tols = {n_: max(1e-9, 300.0 * v) for n_, v in delta.items()}
        tols_lean = {n_: max(tols[n_], min(1e-7, 2e4 * v)) for n_, v in delta.items()}
        gates[seed] = max(tols.values())
        raw = max(raw, (300.0 * max(delta.values()), seed))
        for n_, t in tols.items():
            if not t <= ceiling:
                port_moved.append((seed, n_, f'gate {t:.2e} > ceiling {ceiling:.0e}', info))
            if not tols_lean[n_] <= lean_ceiling:
                port_moved.append((seed, n_, f'lean gate {tols_lean[n_]:.2e} > ceiling {lean_ceiling:.0e}', info))
        for name, (run, lean) in fz.kernels.items():
            g3 = table([run(s) for s in batches])
            for g, w, n_ in zip(g3, w3, names):
                if not _same_nonfinite(g, w, signs):
                    failures.append((seed, name, n_, 'non-finite entries differ', info))
                    continue
                e, tol = _dist_any(g, w, n_, d), (tols_lean if lean else tols)[n_]
                if not e <= tol:
                    failures.append((seed, name, n_, f'{e:.3e} > {tol:.1e}', dict(info, delta=delta[n_])))
                worst[name] = max(worst.get(name, 0.0), e)
                arrays += 1
                below += e < 1e-10
                if e > 1e-9:
                    print(f'  {family} seed {seed} {name} {n_}: {e:.2e}  ({info}; the port under the perturbation: {delta[n_]:.2e})')
    print(f'{family} restarted every {L} steps: {total} segments, {dropped} dropped ({100.0 * dropped / total:.2f} %); largest 300 x delta of the port '
          f'{raw[0]:.2e} (seed {raw[1]}; 2e4 x delta {raw[0] * 2e4 / 300:.2e}), {sum(t > 1e-9 for t in gates.values())} of {len(gates)} sets gated above 1e-9; '
          f'{below} of {arrays} output arrays below 1e-10; worst ' + ', '.join(f'{k_} {v:.2e}' for k_, v in worst.items()))
    assert not port_moved, ('the PORT moved, not the kernels', port_moved[:6])
    assert dropped <= drop_cap * total, ('the PORT moved: share of dropped segments', dropped, total, drop_cap)
    assert not failures, failures[:6]


def test_ekf_restarted_from_the_ports_rows():
    """All 240 sets of the EKF fuzz, restarted from the port's rows every 128 steps (two 64-step chunks: the state machine takes one decision
    from history), through the one-trial, the four-trials and the lane kernel.  Lane gate max(1e-9, 300 delta_seg); the matrix-core kernels
    may also use min(1e-7, 2e4 delta_seg), as in the whole-record test.  The one-trial kernel's counters account for every chunk of every
    segment, and every tier is reached.

    Ceilings (the rule: _run_restarted): C = 1e-8 on max(1e-9, 300 delta_seg), the lane kernel's gate -- no set is held to less than that by a
    full-accuracy kernel -- and C_lean = 1e-7 on the matrix-core kernels' gate, whose min(1e-7, 2e4 delta_seg) term reaches its end of 1e-7 on
    the worst set.  Largest 300 delta_seg of the port: 2.09e-9 (seed 52; 2e4 delta_seg 1.39e-7) on the build host and the same 2.09e-9 (seed 52) on
    the GPU box's host; the larger x 3, rounded up to a power of ten.  Dropped segments (non-finite or non-positive-variance start row):
    219 of 16 811 (1.30 %), capped at 3 %, on both hosts.  Chunks by tier over the run (MI355X): high 6437, common 5767, low 807, mid 4466, wide 7633,
    checked 34, redone 7433 -- every tier is reached at L = 128.

    What this form sees and the whole records do not, tried on scratch builds with one tier's softplus off by 1e-7 relative:
    the whole-record test fails too -- its gate follows the conditioning, and so does a kernel's error -- but on fewer sets: 139 of 240 against 185
    here for the MID tier, 61 against 89 for LOW; of the three sets the whole records gate above 1e-5, this test fails two each time (138 and 199;
    29 and 138), the whole-record test none.  The WIDE tier, where those sets spend 93 % of their chunks, fails 237 sets in both forms."""
    from chirpgp_amd import filters_smoothers as fs, models as pm, _engine
    from oracle import port
    totals = dict.fromkeys(_engine.REGIME_COUNTERS, 0)
    miscounted = []

    def setup(seed):
        B, T, dt, Xi, params, ys, _ = make_set(seed)
        _, _, disc, m0, P0, H = pm.build_chirp_model(params)
        want = port.filter(port.F_EKF, disc, None, H, Xi, m0, P0, dt, ys)
        sign = np.random.default_rng(seed).choice([-1., 1.], size=ys.shape)

        def model(s):
            return pm.build_chirp_model(s.params)[2]

        def counted(s):
            _engine.debug_set(_engine.DBG_COUNT_REGIMES, 1)
            _engine.debug_counters(reset=True)
            got = fs.ekf(model(s), s.H, s.Xi, s.m0, s.P0, dt, s.ys, flags=ONE)
            rg = _engine.debug_counters(reset=True)
            _engine.debug_set(_engine.DBG_COUNT_REGIMES, 0)
            chunks = s.trial.size * ((s.length + 63) // 64)
            kept = rg['high'] + rg['common'] + rg['low'] + rg['mid'] + rg['redone'] + rg['wide'] + rg['checked']
            if kept != chunks:
                miscounted.append((seed, s.length, kept, chunks, rg))
            for k in totals:
                totals[k] += rg[k]
            return got

        return FuzzSet(dict(B=B, T=T, dt=dt), 4, want, m0, P0, params, Xi, H, ys, sign,
                       lambda s, y: port.filter(port.F_EKF, model(s), None, s.H, s.Xi, s.m0, s.P0, dt, y),
                       {'one-trial': (counted, True),
                        'four-trials': (lambda s: fs.ekf(model(s), s.H, s.Xi, s.m0, s.P0, dt, s.ys, flags=FOUR), True),
                        'lane': (lambda s: fs.ekf(model(s), s.H, s.Xi, s.m0, s.P0, dt, s.ys, flags=LANE), False)})

    _run_restarted('ekf', range(N_SETS), 128, setup, ceiling=1e-8, lean_ceiling=1e-7, drop_cap=0.03, signs=True)
    print('chunks by regime over the restarted fuzz:', totals)
    assert not miscounted, miscounted[:6]
    for k in ('high', 'common', 'low', 'mid', 'wide'):
        assert totals[k] > 0, (k, totals)


@pytest.mark.parametrize('config', ['gh3_d4', 'cubature_d8'])
def test_sigma_point_filters_restarted_from_the_ports_rows(config):
    """The 60 sets of the sigma-point fuzz in restarted form: Gauss-Hermite order 3 on the d = 4 model (one wavefront per trial and one lane per
    trial) every 128 steps, the cubature rule on the three-harmonic model (d = 8, tile layout) every 64 steps.  Every kernel here has a lean
    fan, so every one gets max(1e-9, 300 delta_seg, min(1e-7, 2e4 delta_seg)), as in the whole-record test.

    Ceilings: C = C_lean = 1e-6 for both (300 delta_seg exceeds the 1e-7 at which the other term ends).  Largest 300 delta_seg of the port: 6.59e-8 (seed 1035) / 1.07e-7 (seed 1036) on the build
    host, the same 6.59e-8 / 1.07e-7 (same seeds) on the GPU box's host.  Dropped segments: 39 of 2 793 (1.40 %) and 74 of 5 346 (1.38 %), capped at 3 %."""
    from chirpgp_amd import filters_smoothers as fs, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    from oracle import port
    d, L = (4, 128) if config == 'gh3_d4' else (8, 64)
    sgps = SigmaPoints.gauss_hermite(4, 3) if config == 'gh3_d4' else SigmaPoints.cubature(8)
    shapes = ((0x2, 'wave'), (0x4, 'lane')) if config == 'gh3_d4' else ((0x2, 'wave'),)

    def build(params):
        return pm.build_chirp_model(params) if config == 'gh3_d4' else pm.build_harmonic_chirp_model(params, num_harmonics=3)

    def setup(seed):
        B, T, dt, Xi, params, ys, _ = make_set(seed)
        T = min(T, 1200)
        ys = np.ascontiguousarray(ys[:, :T])
        _, _, disc, m0, P0, H = build(params)
        want = port.filter(port.F_SGP, disc, sgps, H, Xi, m0, P0, dt, ys)
        sign = np.random.default_rng(seed - 1000).choice([-1., 1.], size=ys.shape)
        return FuzzSet(dict(B=B, T=T, dt=dt), d, want, m0, P0, params, Xi, H, ys, sign,
                       lambda s, y: port.filter(port.F_SGP, build(s.params)[2], sgps, s.H, s.Xi, s.m0, s.P0, dt, y),
                       {shape: (lambda s, fl=fl: fs.sgp_filter(build(s.params)[2], sgps, s.H, s.Xi, s.m0, s.P0, dt, s.ys, flags=fl), True) for fl, shape in shapes})

    _run_restarted(config, range(1000, 1060), L, setup, ceiling=1e-6, lean_ceiling=1e-6, drop_cap=0.03)


@pytest.mark.parametrize('config', ['cd_ekf', 'cd_sgp_filter'])
def test_continuous_discrete_filters_restarted_from_the_ports_rows(config):
    """The 40 sets of the continuous-discrete fuzz in restarted form, every 128 steps, one wavefront per trial; a segment is compared up to the
    port's first broken-down step in it (_broken_from), and one that breaks down at its first step counts as dropped.

    Ceilings: C = 1e-9 on max(1e-9, 300 delta_seg), which is flat -- 300 delta_seg of the port is 1.01e-11 (cd_ekf) and 8.81e-12 (cd_sgp_filter) on
    the build host, the same 1.01e-11 and 8.81e-12 on the GPU box's host -- and C_lean = 1e-8 on the gate the kernels get, max(1e-9, min(1e-7, 2e4 delta_seg)):
    2e4 delta_seg is 6.7e-10 and 5.9e-10, x 3 and rounded up (the gate itself is 1e-9 on every set today).  Dropped segments: 14 of 1 345 (1.04 %) and 109 of 1 345 (8.10 %), capped at 5 % (cd_ekf) and 15 % (cd_sgp_filter: RK4 breaks down at dt = 1e-2)."""
    import copy
    from chirpgp_amd import filters_smoothers as fs, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    from oracle import port
    gh3 = SigmaPoints.gauss_hermite(4, 3)
    method, sg = (port.F_CD_EKF, None) if config == 'cd_ekf' else (port.F_CD_SGP, gh3)

    def with_gamma(params):
        drift, disp = pm.build_chirp_model(params)[:2]
        dg = copy.copy(drift)
        dg.gamma = disp.outer()
        return drift, disp, dg

    def run(s, dt):
        drift, disp, _ = with_gamma(s.params)
        if config == 'cd_ekf':
            return fs.cd_ekf(drift, disp, s.H, s.Xi, s.m0, s.P0, dt, s.ys, flags=0x2)
        return fs.cd_sgp_filter(drift, disp(None), gh3, s.H, s.Xi, s.m0, s.P0, dt, s.ys, flags=0x2)

    def setup(seed):
        B, T, dt, Xi, params, ys, _ = make_set(seed)
        T = min(T, 800)
        ys = np.ascontiguousarray(ys[:, :T])
        _, _, _, m0, P0, H = pm.build_chirp_model(params)
        want = port.filter(method, with_gamma(params)[2], sg, H, Xi, m0, P0, dt, ys)
        sign = np.random.default_rng(seed - 2000).choice([-1., 1.], size=ys.shape)
        return FuzzSet(dict(B=B, T=T, dt=dt), 4, want, m0, P0, params, Xi, H, ys, sign,
                       lambda s, y: port.filter(method, with_gamma(s.params)[2], sg, s.H, s.Xi, s.m0, s.P0, dt, y),
                       {'wave': (lambda s: run(s, dt), True)})

    _run_restarted(config, range(2000, 2040), 128, setup, ceiling=1e-9, lean_ceiling=1e-8, drop_cap=0.05 if config == 'cd_ekf' else 0.15, until_breakdown=True)


@pytest.mark.parametrize('family', ['lascala', 'harmonic', 'kpt'])
def test_other_models_restarted_from_the_ports_rows(family):
    """The toy-chirp families of test_random_models_through_the_other_kernels in restarted form, every 128 steps (their records have 30 .. 700
    steps): the port alone gates sets of each above 1e-9 on the whole record -- La Scala sgp_filter up to 1e-7, the three-harmonic EKF 3e-9,
    KPT up to 3e-6 -- so each is run again from the port's rows: La Scala (ekf and sgp_filter with Gauss-Hermite order 3, one wavefront per
    trial and one lane per trial), the harmonic models at d = 6 and 8 (ekf, tile layout and per lane) and ekf_for_kpt at d = 3, 4, 5 (tile
    layout, per lane, generic).  Gate as in the whole-record test: max(1e-9, 300 delta_seg, min(1e-7, 2e4 delta_seg)).

    Ceilings (OTHER_CEILINGS: C on max(1e-9, 300 delta_seg), C_lean on the gate the kernels get): 1e-9 / 1e-9 for the La Scala EKF, 1e-9 / 1e-8
    for the harmonic EKF, 1e-8 / 1e-7 for the La Scala sgp_filter, 1e-5 / 1e-5 for KPT.  Largest 300 delta_seg (2e4 delta_seg) of the port:
    La Scala ekf 1.44e-12 (9.6e-11), La Scala sgp_filter 1.56e-9 (1.04e-7; seed 12), harmonic ekf 1.73e-11 (1.15e-9), KPT 6.33e-7 (4.2e-5;
    seed 8, three harmonics, B = 6, T = 253) on the build host; the GPU box's host gives the same four figures.  Dropped segments: none of 182, 221 and 242, capped at 3 %."""
    from chirpgp_amd import filters_smoothers as fs, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    from oracle import port
    gh3 = SigmaPoints.gauss_hermite(4, 3)
    kind = ('lascala', 'harmonic', 'kpt').index(family)

    def setup(seed):
        B, T, sign, _, dt, ysc, _, toy = _random_model_set(seed)
        info = dict(B=B, T=T)
        if family == 'kpt':
            nh, c, yk = toy
            spec = pm.linear_cond_m_cov(c.F, c.Sigma)
            spec.model_id, spec.n_harm = pm.M_KPT, nh
            want = port.filter(port.F_EKF_KPT, spec, None, None, c.Xi, c.m0, c.P0, c.dt, yk)
            return FuzzSet(info, nh + 2, want, c.m0, c.P0, None, c.Xi, None, yk, sign,
                           lambda s, y: port.filter(port.F_EKF_KPT, spec, None, None, s.Xi, s.m0, s.P0, c.dt, y),
                           {name: (lambda s, fl=fl: fs.ekf_for_kpt(c.F, c.Sigma, c.h, s.Xi, s.m0, s.P0, c.dt, s.ys, flags=fl), True)
                            for name, fl in (('wave', 0x2), ('lane', 0x4), ('generic', 0x12))})
        if family == 'harmonic':
            nh, prm = toy

            def build(params):
                return pm.build_harmonic_chirp_model(params, num_harmonics=nh)
            d = 2 * nh + 2
        else:
            prm, build, d = toy, pm.build_lascala_model, 4
        _, _, disc, m0c, P0c, Hc = build(prm)
        want = port.filter(port.F_EKF, disc, None, Hc, 0.1, m0c, P0c, dt, ysc)
        kernels = {f'ekf {name}': (lambda s, fl=fl: fs.ekf(build(s.params)[2], s.H, s.Xi, s.m0, s.P0, dt, s.ys, flags=fl), True)
                   for name, fl in (('wave', 0x2), ('lane', 0x4))}
        return FuzzSet(info, d, want, m0c, P0c, prm, 0.1, Hc, ysc, sign,
                       lambda s, y: port.filter(port.F_EKF, build(s.params)[2], None, s.H, s.Xi, s.m0, s.P0, dt, y), kernels)

    def setup_sgp(seed):
        B, T, sign, _, dt, ysc, _, prm = _random_model_set(seed)
        _, _, disc, m0c, P0c, Hc = pm.build_lascala_model(prm)
        want = port.filter(port.F_SGP, disc, gh3, Hc, 0.1, m0c, P0c, dt, ysc)
        return FuzzSet(dict(B=B, T=T), 4, want, m0c, P0c, prm, 0.1, Hc, ysc, sign,
                       lambda s, y: port.filter(port.F_SGP, pm.build_lascala_model(s.params)[2], gh3, s.H, s.Xi, s.m0, s.P0, dt, y),
                       {f'sgp_filter {name}': (lambda s, fl=fl: fs.sgp_filter(pm.build_lascala_model(s.params)[2], gh3, s.H, s.Xi, s.m0, s.P0, dt, s.ys, flags=fl), True)
                        for name, fl in (('wave', 0x2), ('lane', 0x4))})

    seeds = range(kind, 48, 3)
    ceiling, lean_ceiling = OTHER_CEILINGS[family]
    _run_restarted(f'{family} ekf', seeds, 128, setup, ceiling=ceiling, lean_ceiling=lean_ceiling, drop_cap=0.03)
    if family == 'lascala':
        ceiling, lean_ceiling = OTHER_CEILINGS['lascala sgp_filter']
        _run_restarted('lascala sgp_filter', seeds, 128, setup_sgp, ceiling=ceiling, lean_ceiling=lean_ceiling, drop_cap=0.03)

