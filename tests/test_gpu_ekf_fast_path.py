"""The d = 4 matrix-core EKF takes runs of kept chunks on a loop of their own (cgp_mfma4.hpp: the fast path): behind a chunk kept in the
HIGH or the COMMON tier the following chunks stay on it for as long as each one is full (64 steps), lies behind the burn-in and the
junction of a time-split segment, no sticky count runs and its start state selects the same tier; a chunk whose verdict fails there is
handed back to the general path untouched.  What this file checks is that the hand-overs lose nothing: records that stay on the fast
path, leave it in the middle of a chunk and come back, never get there (LOW, MID starts) or fall through every tier (an `inf`
measurement), at record lengths around the chunk size, with and without NLL rows, with subsets of the outputs and in a time-split launch
whose junction lies where a run would be -- every output against the C port of the reference's recursion at 1e-9 relative to the output's
largest entry (the gate of the full-size parity test), non-finite entries in the same places with the same values, and every launch
between guard bands: all of its outputs written, nothing else.

The port runs once per record set, at the longest length; the recursion is causal, so its first T rows are the reference of length T."""
import functools
import math

import numpy as np
import pytest

from tests import guard_bands as gb

pytestmark = pytest.mark.gpu

GATE = 1e-9
WAVE = 0x2                                  # one trial per wavefront: ekf4_mfma_kernel
B = 3
LENGTHS = (1, 8, 63, 64, 65, 128, 129, 197)
T_MAX = max(LENGTHS)
KINDS = ('high', 'dip', 'low', 'mid', 'inf')
DT = 1e-3
NAMES = ('mfs', 'Pfs', 'nll')


def _tone(freq, seed, Xi):
    return np.sin(2 * math.pi * np.cumsum(freq) * DT) + math.sqrt(Xi) * np.random.default_rng(seed).standard_normal(freq.size)


@functools.lru_cache(maxsize=None)
def _records(kind):
    """-> (model parameters, Xi, records (B, T_MAX)).  Where the frequency state u2 of each goes is asserted on the port's own path in
    _reference below."""
    import bench
    from oracle import np_models as om_
    if kind in ('high', 'inf'):              # 9 - 11 Hz from a start at 9: u2 >= 6.5 at every chunk's start, never below 5
        freq = 10.0 - np.cos(2 * math.pi * np.arange(T_MAX) / T_MAX)
        ys = np.stack([_tone(freq, 11 + i, 0.05) for i in range(B)])
        if kind == 'inf':
            ys[1, 100] = np.inf              # the middle of the second chunk of trial 1
        return (0.1, 0.5, 0.1, 0.3, 1., float(om_.g_inv(9.0))), 0.05, ys
    if kind == 'dip':                        # 9 Hz with 16 steps at 1 Hz inside the second chunk, a short length scale of the frequency prior
        freq = np.full(T_MAX, 9.0)
        freq[68:84] = 1.0
        return (0.1, 0.5, 0.1, 0.1, 1., float(om_.g_inv(9.0))), 0.01, np.stack([_tone(freq, s, 0.01) for s in (2, 3, 4)])
    if kind == 'low':                        # a negative start the filter does not recover from
        return (0.1, 0.1, 0.1, 1., 1., -3.0), 0.1, bench.chirp_batch(B, T_MAX, 5, Xi=0.1, offset=2.0)
    assert kind == 'mid'                     # |u2| < 1.5 at the start
    return (0.1, 0.1, 0.1, 1., 1., 0.5), 0.1, bench.chirp_batch(B, T_MAX, 5, Xi=0.1, offset=1.0)


def _model(kind):
    from chirpgp_amd import models as pm
    p, Xi, ys = _records(kind)
    _, _, disc, m0, P0, H = pm.build_chirp_model(np.array(p))
    return disc, H, Xi, m0, P0, ys


def u2_path(kind):
    """The port's frequency state BEFORE each step (B, T_MAX) -- what the kernel's verdicts look at -- and the largest increment of the
    rotation angle dt 2 pi fs softplus(u2) between two steps, per chunk (B, 4): a chunk is kept on a speculative tier only while it
    stays below 1.5 x 2^-8."""
    want = _reference(kind)
    p, _, _ = _records(kind)
    disc, H, Xi, m0, P0, ys = _model(kind)
    with np.errstate(all='ignore'):
        before = np.concatenate([np.full((B, 1), float(np.asarray(m0).reshape(-1)[2])), want[0][:, :-1, 2]], axis=1)
        d = np.abs(np.diff(DT * 2 * math.pi * p[4] * np.logaddexp(0.0, before), axis=1, prepend=np.nan))
        jump = np.stack([np.fmax.reduce(d[:, a:a + 64], axis=1) for a in range(0, T_MAX, 64)], axis=1)
    return before, jump


BOUND = 1.5 * 2.0 ** -8


def path_facts(kind):
    """What each record is there for, on the port's own path (run on the CPU when the records were chosen, and by every test here)."""
    u2, jump = u2_path(kind)
    starts = u2[:, ::64]                                                   # the state each chunk starts from
    if kind == 'high':
        assert (starts >= 6.5).all() and (u2 >= 5.0).all() and (u2 < 700).all() and (jump < 0.8 * BOUND).all(), (starts, u2.min(), jump)
    elif kind == 'inf':
        assert (starts[:, :2] >= 6.5).all() and (u2[:, :101] >= 5.0).all() and (jump[:, 0] < 0.8 * BOUND).all()
        assert np.isfinite(u2[[0, 2]]).all() and not np.isfinite(u2[1, 101:]).any() and np.isfinite(u2[1, :101]).all()
    elif kind == 'dip':
        # chunk 0 stays in HIGH; chunk 1 starts in HIGH's band, dips below 5 inside and is repeated in COMMON; chunk 2 starts in COMMON's
        # band and stays there -- the run that follows the repeated chunk; the last, short chunk starts back in HIGH's band; no increment
        # of the angle comes near the bound, so the frequency state alone decides
        assert (jump < 0.8 * BOUND).all(), jump
        assert (starts[:, :2] >= 6.5 + 0.2).all() and (u2[:, :64] >= 5.0 + 0.2).all(), (starts, u2[:, :64].min(axis=1))
        assert (u2[:, 64:128].min(axis=1) < 5.0 - 0.2).all() and (u2[:, 64:128] >= 1.5 + 0.2).all(), u2[:, 64:128].min(axis=1)
        assert ((starts[:, 2] >= 1.75 + 0.2) & (starts[:, 2] < 6.5 - 0.2)).all() and (u2[:, 128:192] >= 1.5 + 0.2).all(), starts
        assert (starts[:, 3] >= 6.5 + 0.2).all() and (u2[:, 192:] >= 5.0 + 0.2).all(), starts
    elif kind == 'low':
        assert (starts[:, 0] <= -1.75).all(), starts
    else:
        assert (np.abs(starts[:, 0]) < 1.5).all(), starts
    return True


@functools.lru_cache(maxsize=None)
def _reference(kind):
    from oracle import port
    disc, H, Xi, m0, P0, ys = _model(kind)
    with np.errstate(all='ignore'):
        want = port.filter(port.F_EKF, disc, None, H, Xi, m0, P0, DT, ys)
    for w in want:
        w.setflags(write=False)
    return want


def _err(got, want):
    """max |got - want| over the finite entries / the largest finite |want|; the others (NaN, +-inf) must sit in the same places and
    be the same."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), 'non-finite entries in other places'
    assert np.array_equal(np.isnan(want), np.isnan(got)) and np.array_equal(want[~fin & ~np.isnan(want)], got[~fin & ~np.isnan(want)]), 'other non-finite values'
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin])) / max(np.max(np.abs(want[fin])), 1e-300))


def _launch(kind, T, expect, **kw):
    """One guarded launch on the first T steps -> the outputs; the guard bands intact, every requested output word written."""
    from chirpgp_amd import filters_smoothers as fs
    disc, H, Xi, m0, P0, ys = _model(kind)
    arena = gb.Arena('cuda', 'odd')
    with arena.installed():
        got = fs.ekf(disc, H, Xi, m0, P0, DT, np.ascontiguousarray(ys[:, :T]), **kw)
    assert arena.check() == [], (kind, T, kw)
    if expect is not None:
        assert sorted(n for n, _ in arena.requests) == sorted(expect), (arena.requests, expect)
    return got


def _check_rows(got, want, T, label, rows=slice(None)):
    for g, w, n in zip(got, want, NAMES):
        if g is None:
            continue
        e = _err(np.asarray(g)[:, rows], w[:, :T][:, rows])
        print(label, n, f'{e:.1e}')
        assert e <= GATE, (label, n, e)


@pytest.mark.parametrize('T', LENGTHS)
@pytest.mark.parametrize('kind', KINDS)
def test_every_record_at_every_length(kind, T):
    assert path_facts(kind)
    got = _launch(kind, T, NAMES, flags=WAVE)
    _check_rows(got, _reference(kind), T, f'{kind} T={T}')


def _counted(kind):
    from chirpgp_amd import _engine
    assert path_facts(kind)
    _engine.debug_set(_engine.DBG_COUNT_REGIMES, 1)
    _engine.debug_counters(reset=True)
    try:
        got = _launch(kind, T_MAX, NAMES, flags=WAVE)
        rg = _engine.debug_counters(reset=True)
    finally:
        _engine.debug_set(_engine.DBG_COUNT_REGIMES, 0)
    print(kind, rg)
    _check_rows(got, _reference(kind), T_MAX, kind + ' counted')
    assert rg['high'] + rg['common'] + rg['low'] + rg['mid'] + rg['redone'] + rg['wide'] + rg['checked'] == 4 * B, rg
    return rg


def test_the_high_record_is_kept_in_high_throughout():
    rg = _counted('high')
    assert rg['high'] == 4 * B and rg['high_left'] == 0, rg


def test_the_dip_record_leaves_the_fast_path_and_comes_back():
    """The kernel's own regime counters on the record that dips: per trial, chunk 0 is kept in HIGH, chunk 1 leaves HIGH (once, in the
    general path: the failed pass of the fast path counts nothing) and is kept in COMMON, chunk 2 is kept in COMMON, the short last chunk
    in HIGH -- what the general path alone counts for these records."""
    rg = _counted('dip')
    assert rg['high'] == 2 * B and rg['common'] == 2 * B and rg['high_left'] == B and rg['redone'] == 0, rg


VARIANTS = {
    'nll_final_only': (dict(nll_final_only=True, want=(False, False, True)), ('nll',)),
    'nll_final_with_rows': (dict(nll_final_only=True), NAMES),
    'no_nll': (dict(want=(True, True, False)), ('mfs', 'Pfs')),
    'means_and_nll': (dict(want=(True, False, True)), ('mfs', 'nll')),
    'covariances_only': (dict(want=(False, True, False)), ('Pfs',)),
    'nll_rows_only': (dict(want=(False, False, True)), ('nll',)),
}


@pytest.mark.parametrize('T', (65, 197))
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_launch_variants(variant, kind, T):
    kw, expect = VARIANTS[variant]
    got = _launch(kind, T, expect, flags=WAVE, **kw)
    want = _reference(kind)
    assert [g is not None for g in got] == [n in expect for n in NAMES]
    if kw.get('nll_final_only'):
        _check_rows(got[:2] + (None,), want, T, f'{variant} {kind} T={T}')
        e = _err(got[2], want[2][:, T - 1])
        print(variant, kind, T, 'nll total', f'{e:.1e}')
        assert e <= GATE, (variant, kind, T, e)
    else:
        _check_rows(got, want, T, f'{variant} {kind} T={T}')


@pytest.mark.parametrize('T', (129, 197))
@pytest.mark.parametrize('kind', ('high', 'dip'))
def test_time_split_launch_with_the_junction_inside_a_run(kind, T):
    """time_split = (2, 64): segments of 128 steps, the second one burns in over the chunk at 64, which it keeps, and goes on record at
    128 -- the junction chunk lies where the fast path would go on, and takes the general path.  Segment 0 IS the sequential filter (bit
    for bit against the sequential launch, which is within the gate of the port); segment 1 is the filter started from (m0, P0) at step
    64, so the port run on the record from step 64 on is its reference, the NLL rows continuing from the total of segment 0."""
    from oracle import port
    disc, H, Xi, m0, P0, ys = _model(kind)
    seq = _launch(kind, T, NAMES, flags=WAVE)
    _check_rows(seq, _reference(kind), T, f'sequential {kind} T={T}')
    got = _launch(kind, T, None, time_split=(2, 64), return_junction_error=True)
    err = np.asarray(got[3].cpu()) if hasattr(got[3], 'cpu') else np.asarray(got[3])
    assert err.shape == (B,) and np.isfinite(err).all(), err
    for g, s, n in zip(got[:3], seq, NAMES):
        assert np.array_equal(np.asarray(g)[:, :128], np.asarray(s)[:, :128]), (n, 'segment 0 is not the sequential filter')
    late = port.filter(port.F_EKF, disc, None, H, Xi, m0, P0, DT, np.ascontiguousarray(ys[:, 64:T]))
    want = (late[0][:, 64:], late[1][:, 64:], np.asarray(got[2])[:, 127:128] + (late[2][:, 64:] - late[2][:, 63:64]))
    for g, w, n in zip(got[:3], want, NAMES):
        e = _err(np.asarray(g)[:, 128:], w)
        print('time split', kind, T, n, f'{e:.1e}')
        assert e <= GATE, (kind, T, n, e)
