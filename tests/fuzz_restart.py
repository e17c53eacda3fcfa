"""Restarting a fuzz record set from the reference's own filtering rows (tests/test_gpu_fuzz.py).

A whole random record can amplify a 1e-15 perturbation to 1e-4 (or, for a lost sigma-point filter, to O(1)): the amplification comes from the
length of the record, not from one step, and a gate scaled by it admits anything on exactly the records that live in the rarely used tiers.
Cut into segments of L steps, each started from the PORT's row just before it, the same records exercise the same states of the same tiers
and amplify over L steps at the most -- every (trial, segment) pair becomes one batch entry with its own m0, P0, parameters and Xi.
"""
from collections import namedtuple

import numpy as np

Segments = namedtuple('Segments', 'trial start length m0 P0 params Xi H ys')


def cut(seg, a):
    """The segments' slices of a per-trial, per-step array a (B, T, ...) -> (N, length, ...)."""
    return np.ascontiguousarray(np.asarray(a)[seg.trial[:, None], seg.start[:, None] + np.arange(seg.length)[None, :]])


def restart_batches(want, m0, P0, params, Xi, H, ys, L):
    """One fuzz set -> ([full segments, tails], number of segments, number dropped).

    want = (mfs, Pfs, nll) is the port's whole-record result.  The first batch holds every full segment ys[b, s:s+L], s = 0, L, 2L, ..., the
    second (if T mod L >= 1) every trial's tail of T mod L steps.  A segment at s = 0 starts from the set's own m0[b], P0[b], any other from
    want[0][b, s-1], want[1][b, s-1]; its trial's parameters, Xi (and H, if H is per trial) are carried along.  A segment whose start row is
    non-finite or has a non-positive variance is dropped (nothing follows from it) and counted; one that CONTAINS a NaN or inf measurement
    is kept.  A batch that lost all its segments is left out."""
    mfs, Pfs = np.asarray(want[0]), np.asarray(want[1])
    ys = np.asarray(ys)
    B, T = ys.shape
    d = mfs.shape[-1]
    m0 = np.broadcast_to(np.asarray(m0, dtype=np.float64), (B, d))
    P0 = np.broadcast_to(np.asarray(P0, dtype=np.float64), (B, d, d))
    Xi = np.broadcast_to(np.asarray(Xi, dtype=np.float64), (B,))
    H = None if H is None else np.asarray(H, dtype=np.float64)
    params = None if params is None else np.asarray(params, dtype=np.float64)
    diag = np.arange(d)
    n_full, tail = divmod(T, L)
    batches, total, dropped = [], 0, 0
    for starts, length in ((L * np.arange(n_full), L), (np.array([L * n_full]), tail)):
        if length < 1 or starts.size == 0:
            continue
        trial, start = (a.ravel() for a in np.meshgrid(np.arange(B), starts, indexing='ij'))
        first = start == 0
        prev = np.where(first, 0, start - 1)
        ms = np.where(first[:, None], m0[trial], mfs[trial, prev])
        Ps = np.where(first[:, None, None], P0[trial], Pfs[trial, prev])
        with np.errstate(invalid='ignore'):
            keep = np.isfinite(ms).all(axis=-1) & np.isfinite(Ps).all(axis=(-1, -2)) & (Ps[:, diag, diag] > 0).all(axis=-1)
        total += keep.size
        dropped += int((~keep).sum())
        if not keep.any():
            continue
        trial, start = trial[keep], start[keep]
        seg = Segments(trial, start, length, np.ascontiguousarray(ms[keep]), np.ascontiguousarray(Ps[keep]),
                       None if params is None else np.ascontiguousarray(params[trial] if params.ndim == 2 else params),
                       np.ascontiguousarray(Xi[trial]), H if (H is None or H.ndim == 1) else np.ascontiguousarray(H[trial]), None)
        batches.append(seg._replace(ys=cut(seg, ys)))
    return batches, total, dropped


def rows(arrays, tail_ndim):
    """Per-step outputs of several batches, (N_i, length_i) + tail shape each, as ONE array of rows: a distance taken over it has the set's
    scales, not one segment's."""
    arrays = [np.asarray(a) for a in arrays]
    return np.concatenate([a.reshape((-1,) + a.shape[a.ndim - tail_ndim:]) for a in arrays], axis=0)
