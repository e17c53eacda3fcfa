"""The NumPy oracle of the timed calls (`dts=`, include/chirpgp_hip_timed.h): one interval per step.

The timed oracle IS the project's oracle (oracle/np_filters.py), driven one step at a time with that step's interval -- no formula is
restated here:
    filter, step t:          fn(..., m, P, dts[t], ys[t:t+1])          one-sample run from the previous filtering result
    smoother, step t+1 -> t: fn(..., [mf_t, ms_{t+1}], [Pf_t, Ps_{t+1}], dts[t+1])[0]
On a constant grid both are the plain oracle bit for bit (tests/test_times_host.py).  With `missing='skip'` the one-sample run is
tests/gap_oracle.py's.  `substeps=n` is the refined-grid definition of tests/substeps_oracle.py with dts[t] / n repeated n times."""
import numpy as np

from tests import gap_oracle as go
from tests import substeps_oracle as so


def grid(T, dt, a, seed=5, long_at=None, zero_at=None):
    """dts = dt (1 + a u), u uniform in (-1, 1) from default_rng(seed); optionally one interval of 3 dt and one of 0."""
    dts = dt * (1.0 + a * np.random.default_rng(seed).uniform(-1.0, 1.0, T))
    if long_at is not None and long_at < T:
        dts[long_at] = 3.0 * dt
    if zero_at is not None and zero_at < T:
        dts[zero_at] = 0.0
    return dts


def run_filter(fn, *args, skip=False):
    """An oracle filter of np_filters (cd_ekf, cd_sgp_filter) on its own time grid.  `args` as the oracle takes them, with the intervals
    (T,) where it takes dt: (..., m0, P0, dts, ys).  skip: NaN samples are gaps.  -> (mfs, Pfs, cumulative nll)."""
    *head, m0, P0, dts, ys = args
    dts, ys = np.asarray(dts, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    assert dts.shape == ys.shape and ys.ndim == 1
    T, d = ys.size, np.size(m0)
    mfs, Pfs, nlls = np.zeros((T, d)), np.zeros((T, d, d)), np.zeros(T)
    m, P, nll = np.asarray(m0, dtype=np.float64), np.asarray(P0, dtype=np.float64), 0.
    for t in range(T):
        one = (*head, m, P, dts[t], ys[t:t + 1])
        mf, Pf, inc = go.gapped(fn, *one) if skip else fn(*one)
        m, P = mf[0], Pf[0]
        nll = nll + inc[0]
        mfs[t], Pfs[t], nlls[t] = m, P, nll
    return mfs, Pfs, nlls


def run_smoother(fn, *args):
    """An oracle smoother of np_filters (cd_eks, cd_sgp_smoother) on its own time grid: (..., mfs, Pfs, dts); dts[0] is never read."""
    *head, mfs, Pfs, dts = args
    mfs, Pfs, dts = np.asarray(mfs, dtype=np.float64), np.asarray(Pfs, dtype=np.float64), np.asarray(dts, dtype=np.float64)
    T = mfs.shape[0]
    assert dts.shape == (T,)
    mss, Pss = mfs.copy(), Pfs.copy()
    for t in range(T - 2, -1, -1):
        m2, P2 = fn(*head, np.stack([mfs[t], mss[t + 1]]), np.stack([Pfs[t], Pss[t + 1]]), dts[t + 1])
        mss[t], Pss[t] = m2[0], P2[0]
    return mss, Pss


def refine_grid(dts, n):
    """(T,) -> (n T,): every interval cut into n equal ones, dts[t] / n repeated n times."""
    return np.repeat(np.asarray(dts, dtype=np.float64) / n, n)


def run_filter_substeps(fn, n, *args):
    """The timed filter with n substeps: the timed oracle on the refined record (NaN at the inserted times, skipped) over the refined grid.
    NaN of the caller's record are real gaps on top.  -> (the caller's T rows, all n T rows: what the smoother needs)."""
    *head, dts, ys = args
    full = run_filter(fn, *head, refine_grid(dts, n), so.refine(ys, n), skip=True)
    return tuple(a[so.kept(n)] for a in full), full


def run_smoother_substeps(fn, n, *args):
    """The timed smoother with n substeps, on the n T filtering rows of run_filter_substeps.  -> (mss, Pss) at the caller's T rows."""
    *head, dts = args
    return tuple(a[so.kept(n)] for a in run_smoother(fn, *head, refine_grid(dts, n)))
