"""The NumPy oracle of `substeps=n` (CGP_RK4_SUBSTEPS, include/chirpgp_hip.h): n RK4 steps of dt / n between two measurements.

The definition is the emulation the engine already offers: refine the record n times with NaN at the inserted times, run the existing
method at step dt / n with the NaN measurements skipped (tests/gap_oracle.py), keep rows n - 1, 2 n - 1, ...  A smoother runs on ALL n T
filtering rows of that refined run, and its rows n - 1, 2 n - 1, ... are kept.  n = 1 is the plain oracle, bit for bit: the record is its
own refinement, dt / 1 is dt, and without a NaN gap_oracle's update is the oracle's."""
import math

import numpy as np

from tests import gap_oracle as go


def chirp_record(f0, T=150, dt=1e-2, Xi=0.1, seed=1):
    """The coarsely sampled records of the tests: sin(2 pi (f0 t + t^2)) + noise of variance Xi at t = dt, 2 dt, ..., T dt."""
    ts = dt * np.arange(1, T + 1)
    return np.sin(2 * math.pi * (f0 * ts + ts ** 2)) + math.sqrt(Xi) * np.random.default_rng(seed).standard_normal(T)


def chirp_params(f0):
    """The chirp model of those records: the demos' start point with the frequency state started at f0."""
    from oracle import np_models as om
    return np.array([0.1, 0.1, 0.1, 1., 1., om.g_inv(f0)])


def chirp_model(f0):
    """(drift, dispersion, discretisation, m0, P0, H) of the oracle for chirp_params(f0)."""
    from oracle import np_models as om
    return om.build_chirp_model(chirp_params(f0))


def refine(ys, n):
    """(T,) -> (n T,): ys at rows n - 1, 2 n - 1, ..., NaN (a missing sample) everywhere else."""
    ys = np.asarray(ys, dtype=np.float64)
    out = np.full(n * ys.size, np.nan)
    out[n - 1::n] = ys
    return out


def kept(n):
    """The rows of a refined run that are the caller's samples."""
    return slice(n - 1, None, n)


def run_filter(fn, n, *args):
    """An oracle filter of np_filters (cd_ekf, cd_sgp_filter) with n substeps.  `args` as the oracle takes them: (..., dt, ys); NaN in ys
    are real gaps on top.  -> ((mfs, Pfs, nll) at the caller's T rows, the same at all n T rows: what the smoother needs)."""
    *head, dt, ys = args
    full = go.gapped(fn, *head, dt / n, refine(ys, n))
    return tuple(np.asarray(a)[kept(n)] for a in full), full


def run_smoother(fn, n, *args):
    """An oracle smoother of np_filters (cd_eks, cd_sgp_smoother) with n substeps.  `args` as the oracle takes them: (..., mfs, Pfs, dt), with
    the n T filtering rows of run_filter's refined run.  -> (mss, Pss) at the caller's T rows."""
    *head, dt = args
    return tuple(np.asarray(a)[kept(n)] for a in fn(*head, dt / n))


def value_and_grad(build, theta, ys, Xi, dt, n, H=None):
    """cd_ekf's final NLL with n substeps and its exact gradient in float64: tests/cd_grad_oracle.py on the refined record at dt / n with the
    NaN samples (the inserted ones, and the record's own) skipped.  build: 'chirp' | 'lascala'.  -> (nll, grad (P,))."""
    from tests import cd_grad_oracle as cgo
    nll, grad = cgo.value_and_grad(build, theta, refine(ys, n), Xi, dt / n, H=H, skip_missing=True)
    return float(nll[-1]), grad[-1]


def gap_emulation(run, n, ys, dt, **kw):
    """The same emulation on the engine: `run(ys, dt, **kw)` is a filter of chirpgp_amd.filters_smoothers closed over everything but the
    record and the step.  ys (T,) or (B, T).  -> the outputs at the caller's rows, and at all n T rows."""
    ys = np.asarray(ys, dtype=np.float64)
    ref = np.full(ys.shape[:-1] + (n * ys.shape[-1],), np.nan)
    ref[..., n - 1::n] = ys
    full = run(ref, dt / n, missing='skip', **kw)
    rows = (slice(None),) * (ys.ndim - 1) + (kept(n),)      # time is the record's last axis and every output's axis of that number
    return tuple(None if a is None else a[rows] for a in full), full
