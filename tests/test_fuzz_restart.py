"""tests/fuzz_restart.py decides what the restarted fuzz compares: its segments, start rows and drops, checked on a hand-made record set."""
import numpy as np

from tests import fuzz_restart as fr


def _set(B=3, T=11, d=2):
    rng = np.random.default_rng(0)
    mfs = rng.standard_normal((B, T, d))
    Pfs = np.tile(np.eye(d), (B, T, 1, 1)) * rng.uniform(0.5, 2.0, size=(B, T, 1, 1))
    ys = rng.standard_normal((B, T))
    m0, P0 = rng.standard_normal((B, d)), np.tile(2.0 * np.eye(d), (B, 1, 1))
    return (mfs, Pfs, np.zeros((B, T))), m0, P0, rng.standard_normal((B, 5)), rng.uniform(0.1, 1.0, size=B), np.array([0., 1.]), ys


def test_segments_start_from_the_row_before_them_and_carry_their_trial():
    want, m0, P0, params, Xi, H, ys = _set()
    (full, tail), total, dropped = fr.restart_batches(want, m0, P0, params, Xi, H, ys, 4)
    assert (total, dropped) == (3 * 2 + 3, 0)
    assert full.length == 4 and tail.length == 3 and full.ys.shape == (6, 4) and tail.ys.shape == (3, 3)
    for seg in (full, tail):
        for k, (b, s) in enumerate(zip(seg.trial, seg.start)):
            np.testing.assert_array_equal(seg.ys[k], ys[b, s:s + seg.length])
            np.testing.assert_array_equal(seg.m0[k], m0[b] if s == 0 else want[0][b, s - 1])
            np.testing.assert_array_equal(seg.P0[k], P0[b] if s == 0 else want[1][b, s - 1])
            np.testing.assert_array_equal(seg.params[k], params[b])
            assert seg.Xi[k] == Xi[b]
        assert seg.H is H or np.array_equal(seg.H, H)
    assert sorted(zip(full.trial, full.start)) == [(b, s) for b in range(3) for s in (0, 4)]
    assert sorted(zip(tail.trial, tail.start)) == [(b, 8) for b in range(3)]
    np.testing.assert_array_equal(fr.cut(tail, want[0]), np.stack([want[0][b, 8:11] for b in tail.trial]))


def test_shared_m0_P0_Xi_are_broadcast_and_no_tail_without_a_remainder():
    want, m0, P0, _, _, _, ys = _set(T=8)
    batches, total, dropped = fr.restart_batches(want, m0[0], P0[0], None, 0.1, None, ys, 4)
    assert len(batches) == 1 and (total, dropped) == (6, 0)
    seg = batches[0]
    assert seg.params is None and seg.H is None and np.array_equal(seg.Xi, np.full(6, 0.1))
    assert all(np.array_equal(seg.m0[k], m0[0]) for k in np.flatnonzero(seg.start == 0))


def test_a_bad_start_row_drops_its_segment_and_a_bad_measurement_does_not():
    want, m0, P0, params, Xi, H, ys = _set()
    want[0][0, 3, 1] = np.nan            # trial 0's segment at s = 4 starts from a NaN mean
    want[1][1, 7, 0, 0] = -1e-3          # trial 1's tail from a negative variance
    want[1][2, 7, 1, 0] = np.inf         # trial 2's tail from an inf covariance entry
    want[1][2, 5, 0, 0] = -1.0           # not a start row: nothing follows from it
    ys[1, 5] = np.nan
    ys[2, 1] = np.inf
    (full, tail), total, dropped = fr.restart_batches(want, m0, P0, params, Xi, H, ys, 4)
    assert (total, dropped) == (9, 3)
    assert sorted(zip(full.trial, full.start)) == [(0, 0), (1, 0), (1, 4), (2, 0), (2, 4)]
    assert list(zip(tail.trial, tail.start)) == [(0, 8)]
    assert np.isnan(full.ys).sum() == 1 and np.isinf(full.ys).sum() == 1


def test_rows_puts_all_segments_of_a_set_into_one_array():
    a, b = np.arange(24.).reshape(2, 3, 4), np.arange(8.).reshape(1, 2, 4)
    assert fr.rows([a, b], 1).shape == (8, 4) and fr.rows([a[..., 0], b[..., 0]], 0).shape == (8,)
    assert fr.rows([np.zeros((2, 3, 4, 4)), np.zeros((1, 2, 4, 4))], 2).shape == (8, 4, 4)
