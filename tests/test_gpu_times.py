"""`dts=` (include/chirpgp_hip_timed.h: cgp_filter_timed, cgp_smoother_timed) on the GPU: cd_ekf, cd_sgp_filter, cd_eks and cd_sgp_smoother
with one interval per step, against the timed NumPy oracle (tests/times_oracle.py: the project's oracle driven one step at a time).

Grids: dts = dt (1 + a u), u = default_rng(5).uniform(-1, 1, T).  The chirp (T = 130), La Scala (T = 130) and the three-harmonic model at
d = 8 (T = 65) at dt = 1e-3 with a = 0.75, one interval of 3 dt (dts[40]) and one of zero (dts[30]: two samples at one instant); the linear
SDE at d = 3 (T = 65, dt = 1e-2) with a = 0.25 and no long interval -- its cd_sgp_smoother oracle goes NaN from 1.5 dt on a regular grid
already -- and the zero interval kept, its oracle staying finite (asserted).  Every test asserts that the oracle's rows are finite first.
The second and third record of a batch have grids of their own, seeds 7 and 9 with the zero interval two and four steps later (on seeds 6
and 8 the d = 8 sigma-point ORACLE leaves the reals at the 3 dt interval: the RK4 step is at its limit there, whoever takes it).

Shapes: T = 1, 2, 64, 65 and 130 (the ends of the kernels' 64-step chunks, a smoother's dts[t + 1] crossing a chunk boundary), B = 1 and 3
(three different records, each with a grid of its own -- (R, T), dts_stride = T -- and again sharing one, dts_stride = 0), the route the call
takes, one lane per trial and the forced generic wave kernel.  Gate: max_rel_err <= 1e-9, the project's (tests/test_gpu_gaps.py: GATE).

Every test here but test_the_grids_are_the_documented_ones, which only builds the grids, fails on the parent commit: the keyword, the
header and the two symbols do not exist there."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import cases as cs
from tests import gap_oracle as go
from tests import substeps_oracle as so
from tests import times_oracle as to

pytestmark = pytest.mark.gpu

GATE = 1e-9
WAVE, THREAD, GENERIC = 0x2, 0x4, 0x10
LENGTHS = (1, 2, 64, 65, 130)
SHAPES = ((0, 'default'), (THREAD, 'lane'), (GENERIC | WAVE, 'generic-wave'))


def _fs():
    from chirpgp_amd import filters_smoothers as fs
    return fs


def three_records(ys):
    """Three different records of one length: a batch whose trials cannot be mistaken for one another."""
    rng = np.random.default_rng(7)
    return np.stack([ys, ys + 0.05 * rng.standard_normal(ys.size), ys[::-1].copy()])


class Setup:
    """One (model, method): the engine's filter and smoother closed over everything but the record, the intervals and the keywords, the
    oracle's pair in the oracle's own argument order, and the model's three time grids (the first is the one the docstring describes)."""
    def __init__(self, c, method, sg, a, long_at, zero_at):
        from oracle import np_filters as onp
        fs = _fs()
        self.c, self.sig = c, method == 'cd_sgp'
        T = c.ys.size
        self.grids = np.stack([to.grid(T, c.dt, a, seed=(5, 7, 9)[k], long_at=long_at, zero_at=None if zero_at is None else zero_at + 2 * k) for k in range(3)])
        if self.sig:
            b, ob, head, ohead = c.disp(None), c.o_disp(None), (sg,), (cs.osig(sg),)
            f, s, self.of, self.os = fs.cd_sgp_filter, fs.cd_sgp_smoother, onp.cd_sgp_filter, onp.cd_sgp_smoother
        else:
            b, ob, head, ohead = c.disp, c.o_disp, (), ()
            f, s, self.of, self.os = fs.cd_ekf, fs.cd_eks, onp.cd_ekf, onp.cd_eks
        self.run = lambda ys, dts, **kw: f(c.drift, b, *head, c.H, c.Xi, c.m0, c.P0, None, ys, dts=dts, **kw)
        self.run_plain = lambda ys, dt=c.dt, **kw: f(c.drift, b, *head, c.H, c.Xi, c.m0, c.P0, dt, ys, **kw)
        self.smooth = lambda mf, Pf, dts, **kw: s(c.drift, b, *head, mf, Pf, None, dts=dts, **kw)
        self.smooth_plain = lambda mf, Pf, dt=c.dt, **kw: s(c.drift, b, *head, mf, Pf, dt, **kw)
        self.ofilter = lambda dts, ys, skip=False: to.run_filter(self.of, c.o_drift, ob, *ohead, c.H, c.Xi, c.m0, c.P0, dts, ys, skip=skip)
        self.osmooth = lambda mf, Pf, dts: to.run_smoother(self.os, c.o_drift, ob, *ohead, mf, Pf, dts)
        self.ofilter_sub = lambda n, dts, ys: to.run_filter_substeps(self.of, n, c.o_drift, ob, *ohead, c.H, c.Xi, c.m0, c.P0, dts, ys)
        self.osmooth_sub = lambda n, mf, Pf, dts: to.run_smoother_substeps(self.os, n, c.o_drift, ob, *ohead, mf, Pf, dts)


@functools.lru_cache(maxsize=None)
def setup(model, method):
    from chirpgp_amd.quadratures import SigmaPoints
    if model == 'chirp':
        return Setup(cs.chirp_case(T=130), method, SigmaPoints.cubature(4), 0.75, 40, 30)
    if model == 'chirp-gh3':
        return Setup(cs.chirp_case(T=130), method, SigmaPoints.gauss_hermite(4, 3), 0.75, 40, 30)
    if model == 'lascala':
        return Setup(cs.lascala_case(T=130), method, SigmaPoints.cubature(4), 0.75, 40, 30)
    if model == 'harm3':
        c = cs.harmonic_case(nh=3, T=65)
        return Setup(c, method, c.sgps, 0.75, 40, 30)
    if model == 'linear3':
        return Setup(cs.linear_case(0, T=65), method, SigmaPoints.cubature(3), 0.25, None, 30)
    raise ValueError(model)


def frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def oracle_filter(model, method, B, shared=False):
    """The timed oracle on the first B of the three records, record b on grid b (shared: all on grid 0); computed once, never written to."""
    s = setup(model, method)
    rows = [s.ofilter(s.grids[0 if shared else b], y) for b, y in enumerate(three_records(s.c.ys)[:B])]
    return frozen(tuple(np.stack([r[i] for r in rows]) for i in range(3)))


@functools.lru_cache(maxsize=None)
def oracle_smoother(model, method, B, T, shared=False):
    """The timed smoother oracle on the first T of the oracle's own filtering rows."""
    s = setup(model, method)
    mf, Pf, _ = oracle_filter(model, method, B, shared)
    rows = [s.osmooth(mf[b, :T], Pf[b, :T], s.grids[0 if shared else b][:T]) for b in range(B)]
    return frozen(tuple(np.stack([r[i] for r in rows]) for i in range(2)))


def worst(got, want, what):
    errs = [cs.max_rel_err(g, w) for g, w in zip(got, want)]
    print(f'{what}: max_rel_err {max(errs):.2e}')
    return max(errs)


def grids_of(s, B, T, shared):
    return np.array(s.grids[0, :T] if shared or B == 1 else s.grids[:B, :T])


MODELS = [('chirp', 'cd_ekf'), ('chirp', 'cd_sgp'), ('chirp-gh3', 'cd_sgp'), ('lascala', 'cd_ekf'), ('lascala', 'cd_sgp'),
          ('harm3', 'cd_ekf'), ('harm3', 'cd_sgp'), ('linear3', 'cd_ekf'), ('linear3', 'cd_sgp')]


def test_the_grids_are_the_documented_ones():
    s = setup('chirp', 'cd_ekf')
    g = s.grids[0]
    want = 1e-3 * (1.0 + 0.75 * np.random.default_rng(5).uniform(-1.0, 1.0, 130))
    keep = np.ones(130, dtype=bool)
    keep[[30, 40]] = False
    assert np.array_equal(g[keep], want[keep]) and g[40] == 3e-3 and g[30] == 0.0 and (g >= 0).all()
    lin = setup('linear3', 'cd_sgp').grids[0]
    assert lin.max() <= 1.25e-2 and lin[30] == 0.0


# ---- filters against the oracle: every length, every launch shape, one grid per record and one shared grid
@pytest.mark.parametrize('model,method', MODELS, ids=[f'{m}-{f}' for m, f in MODELS])
@pytest.mark.parametrize('B,shared', [(1, False), (3, False), (3, True)], ids=['b1', 'b3-own-grids', 'b3-shared-grid'])
def test_filter_parity(model, method, B, shared):
    s = setup(model, method)
    want = oracle_filter(model, method, B, shared)
    assert all(np.isfinite(w).all() for w in want)
    ys = three_records(s.c.ys)[:B]
    for T in (t for t in LENGTHS if t <= ys.shape[1]):
        for flags, shape in SHAPES:
            got = s.run(np.array(ys[:, :T]), grids_of(s, B, T, shared), flags=flags)
            err = worst(got, [w[:, :T] for w in want], f'{model} {method} B={B} shared={shared} T={T} {shape}')
            assert err <= GATE, (T, shape, err)


# ---- smoothers against the oracle, on the oracle's filtering rows, so that their error is their own
@pytest.mark.parametrize('model,method', MODELS, ids=[f'{m}-{f}' for m, f in MODELS])
@pytest.mark.parametrize('B,shared', [(1, False), (3, False), (3, True)], ids=['b1', 'b3-own-grids', 'b3-shared-grid'])
def test_smoother_parity(model, method, B, shared):
    s = setup(model, method)
    mf, Pf, _ = oracle_filter(model, method, B, shared)
    for T in (t for t in LENGTHS if t <= mf.shape[1]):
        want = oracle_smoother(model, method, B, T, shared)
        assert all(np.isfinite(w).all() for w in want)
        for flags, shape in SHAPES:
            got = s.smooth(np.array(mf[:, :T]), np.array(Pf[:, :T]), grids_of(s, B, T, shared), flags=flags)
            err = worst(got, want, f'{model} {method} smoother B={B} shared={shared} T={T} {shape}')
            assert err <= GATE, (T, shape, err)
            # filters_smoothers.py:140-142: the last smoothing row is the last filtering row, verbatim
            assert np.array_equal(got[0][:, -1], mf[:, T - 1]) and np.array_equal(got[1][:, -1], Pf[:, T - 1])


# ---- a constant grid is the plain call: the same step arithmetic, the same h -- the same bits
@pytest.mark.parametrize('model,method', [('chirp', 'cd_ekf'), ('chirp-gh3', 'cd_sgp'), ('harm3', 'cd_ekf'), ('linear3', 'cd_sgp')])
@pytest.mark.parametrize('n', [1, 3])
def test_constant_grid_is_the_plain_call(model, method, n):
    s = setup(model, method)
    ys = three_records(s.c.ys)
    T = ys.shape[1]
    const = np.full(T, s.c.dt)
    for flags, shape in SHAPES:
        plain = s.run_plain(ys, substeps=n, flags=flags)
        timed = s.run(ys, const, substeps=n, flags=flags)
        for k, (a, b) in enumerate(zip(timed, plain)):
            assert np.array_equal(a, b, equal_nan=True), (shape, 'filter output', k, cs.max_rel_err(a, b))
        if n > 1 and flags & THREAD:                        # (substeps run a smoother one wavefront per trial only)
            continue
        splain = s.smooth_plain(plain[0], plain[1], substeps=n, flags=flags)
        stimed = s.smooth(plain[0], plain[1], np.stack([const] * 3), substeps=n, flags=flags)
        for k, (a, b) in enumerate(zip(stimed, splain)):
            assert np.array_equal(a, b, equal_nan=True), (shape, 'smoother output', k, cs.max_rel_err(a, b))


# ---- substeps: the timed call on the refined record with gaps at the inserted times, and the refined-grid oracle
@pytest.mark.parametrize('method', ['cd_ekf', 'cd_sgp'])
@pytest.mark.parametrize('n', [2, 3, 16])
def test_substeps_compose(method, n):
    s = setup('chirp', method)
    T = 65
    ys = three_records(s.c.ys)[:, :T]
    dts = np.array(s.grids[:, :T])
    fine = np.stack([to.refine_grid(g, n) for g in dts])
    ref = np.stack([so.refine(y, n) for y in ys])
    for flags, shape in SHAPES:
        got = s.run(ys, dts, substeps=n, flags=flags)
        full = s.run(ref, fine, missing='skip', flags=flags)
        assert all(np.isfinite(a).all() for a in full)
        assert worst(got, [a[:, so.kept(n)] for a in full], f'{method} n={n} {shape} against the refined timed record') <= GATE
    want, ofull = s.ofilter_sub(n, dts[0], ys[0])
    assert all(np.isfinite(w).all() for w in want)
    got = s.run(ys, dts, substeps=n)
    assert worst([g[0] for g in got], want, f'{method} n={n} against the refined-grid oracle') <= GATE
    # the smoother: on the engine's own rows against the emulation's, every n-th row kept; and against the oracle on the oracle's rows
    full = s.run(ref, fine, missing='skip')
    want_s = [a[:, so.kept(n)] for a in s.smooth(full[0], full[1], fine)]
    assert worst(s.smooth(got[0], got[1], dts, substeps=n), want_s, f'{method} smoother n={n} against the refined timed record') <= GATE
    want_o = s.osmooth_sub(n, ofull[0], ofull[1], dts[0])
    assert all(np.isfinite(w).all() for w in want_o)
    got_o = s.smooth(np.array(want[0]), np.array(want[1]), dts[0], substeps=n)
    assert worst(got_o, want_o, f'{method} smoother n={n} against the refined-grid oracle') <= GATE


@pytest.mark.parametrize('method,n,flags', [('cd_ekf', 1, 0), ('cd_ekf', 3, THREAD), ('cd_sgp', 2, 0), ('cd_sgp', 1, THREAD), ('cd_ekf', 2, GENERIC | WAVE)])
def test_real_gaps_on_top(method, n, flags):
    s = setup('chirp', method)
    spans = ((0, 1), (5, 12), (29, 32), (63, 65), (120, 130))
    ys = np.stack([go.with_gaps(s.c.ys, spans), s.c.ys, go.with_gaps(s.c.ys, spans, 3)])
    rows = [s.ofilter_sub(n, g, y)[0] for g, y in zip(s.grids, ys)]
    want = tuple(np.stack([r[i] for r in rows]) for i in range(3))
    assert all(np.isfinite(w).all() for w in want)
    got = s.run(ys, s.grids, substeps=n, missing='skip', flags=flags)
    assert worst(got, want, f'{method} n={n} with real gaps') <= GATE
    gap = np.isnan(ys)
    prev = np.concatenate([np.zeros((3, 1)), got[2][:, :-1]], axis=1)
    assert np.array_equal(got[2][gap], prev[gap])          # the cumulative NLL holds over a gap


def test_a_zero_interval_is_the_identity():
    """dts[t] = 0: the prediction is the previous filtering result, bit for bit -- the update then conditions it on a second sample."""
    s = setup('chirp', 'cd_ekf')
    T = 40
    got = s.run(s.c.ys[:T], s.grids[0, :T])
    want = oracle_filter('chirp', 'cd_ekf', 1)
    assert s.grids[0, 30] == 0.0 and worst(got, [w[0, :T] for w in want], 'zero interval') <= GATE
    # a record of two samples at one instant: the second step's prediction is the first step's result
    from oracle import np_filters as onp
    two = s.run(s.c.ys[29:31], np.array([s.grids[0, 0], 0.0]))
    upd = onp._linear_update(two[0][0], two[1][0], s.c.H, s.c.Xi, s.c.ys[30])
    assert cs.max_rel_err(two[0][1], upd[0]) <= GATE and cs.max_rel_err(two[1][1], upd[1]) <= GATE


# ---- smoothers: T = 1, select=, a batch beyond a 64-trial block on one wavefront per trial
def test_smoother_single_row_and_select():
    for method in ('cd_ekf', 'cd_sgp'):
        s = setup('chirp', method)
        mf, Pf, _ = oracle_filter('chirp', method, 3)
        one = s.smooth(np.array(mf[:, :1]), np.array(Pf[:, :1]), np.array(s.grids[:, :1]))
        assert np.array_equal(one[0], mf[:, :1]) and np.array_equal(one[1], Pf[:, :1])
        T = 65
        m, P, dts = np.array(mf[:, :T]), np.array(Pf[:, :T]), np.array(s.grids[:, :T])
        mss, Pss = s.smooth(m, P, dts)
        sel = dict(comp=2, mean=True, var=True, expect='softplus', order=10)
        m2, P2, picked = s.smooth(m, P, dts, select=sel)
        assert np.array_equal(m2, mss) and np.array_equal(P2, Pss)
        assert np.array_equal(picked.mean, mss[..., 2]) and np.array_equal(picked.var, Pss[..., 2, 2])
        none_m, none_P, alone = s.smooth(m, P, dts, select=sel, want=(False, False))      # (rows of its own behind the scenes)
        assert none_m is None and none_P is None
        assert all(np.array_equal(alone[k], picked[k]) for k in ('mean', 'var', 'expect'))
        plain = s.smooth_plain(m, P, select=sel)[2]
        assert not np.array_equal(plain.mean, picked.mean)      # the intervals reached the kernel


def test_smoother_batch_of_70():
    """B = 70 with one wavefront per trial, three grids addressed through an index (dts_index) and again as 70 rows of their own."""
    s = setup('chirp', 'cd_ekf')
    T = 64
    mf, Pf, _ = oracle_filter('chirp', 'cd_ekf', 3)
    want = oracle_smoother('chirp', 'cd_ekf', 3, T)
    assert all(np.isfinite(w).all() for w in want)
    idx = np.arange(70) % 3
    m, P = np.array(mf[idx, :T]), np.array(Pf[idx, :T])
    dts = np.array(s.grids[:, :T])
    for flags in (WAVE, THREAD):
        got = s.smooth(m, P, dts, record_index=idx, flags=flags)
        assert worst(got, [w[idx] for w in want], f'cd_eks B=70 indexed grids flags={flags}') <= GATE
        got2 = s.smooth(m, P, np.array(dts[idx]), flags=flags)
        assert all(np.array_equal(a, b) for a, b in zip(got, got2))


# ---- addressing: every probe of a record reads the one copy of its grid
def test_addressing_of_parameter_sweeps():
    from chirpgp_amd import mle
    from chirpgp_amd import models as pm
    s = setup('chirp', 'cd_ekf')
    ys, dts = three_records(s.c.ys), s.grids
    p0 = np.array([0.1, 0.1, 0.1, 1., 1., 7.])
    thetas = pm.g_inv(np.stack([p0 * (1.0 + 0.03 * k) for k in range(7)]))
    got = mle.batched_nll('cd_ekf', pm.build_chirp_model, thetas, ys[0], 0.1, None, dts=dts[0])
    single = np.array([mle.batched_nll('cd_ekf', pm.build_chirp_model, th[None], ys[0], 0.1, None, dts=dts[0])[0] for th in thetas])
    assert np.isfinite(single).all() and np.array_equal(got, single)
    # an indexed subset of the records, each with its own grid: 2 records x 3 rows
    idx = np.array([2, 0])
    got = mle.batched_nll('cd_ekf', pm.build_chirp_model, thetas[:6], ys, 0.1, None, record_index=idx, dts=dts)
    want = np.array([mle.batched_nll('cd_ekf', pm.build_chirp_model, thetas[k][None], ys[idx[k // 3]], 0.1, None, dts=dts[idx[k // 3]])[0] for k in range(6)])
    assert np.isfinite(want).all() and np.array_equal(got, want)
    assert not np.array_equal(got, mle.batched_nll('cd_ekf', pm.build_chirp_model, thetas[:6], ys, 0.1, None, record_index=idx, dts=dts[0]))


def test_device_grids_are_checked_unless_the_caller_has():
    """A CUDA tensor of intervals is copied to the host and checked by every call; check_dts=False (mle's searches, which check once) skips it."""
    import torch
    s = setup('chirp', 'cd_ekf')
    ys = torch.from_numpy(s.c.ys.copy()).cuda()
    dts = torch.from_numpy(s.grids[0].copy()).cuda()
    first, second = s.run(ys, dts), s.run(ys, dts, check_dts=False)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    dts[7] = -1.0
    with pytest.raises(ValueError, match=r'dts\[7\]'):
        s.run(ys, dts)
    with pytest.raises(ValueError, match='T = 65'):
        s.run(ys[:65], dts, check_dts=False)            # (shapes are checked all the same)


# ---- stores: every row of every output, nothing else
@pytest.mark.parametrize('T,B,flags', [(1, 1, 0), (65, 3, 0), (130, 3, 0), (1, 3, THREAD), (65, 3, THREAD), (130, 70, THREAD)])
def test_stores(T, B, flags):
    import torch
    from tests import guard_bands as gb
    for method in ('cd_ekf', 'cd_sgp'):
        s = setup('chirp', method)
        pick = np.arange(B) % 3
        ys = torch.from_numpy(three_records(s.c.ys)[pick, :T].copy()).cuda()
        dts = np.array(s.grids[pick, :T]) if B > 1 else np.array(s.grids[0, :T])
        arena = gb.Arena('cuda', 'aligned')
        with arena.installed():
            mf, Pf, nll = s.run(ys, dts, flags=flags)
            s.smooth(mf, Pf, dts, flags=flags)
        assert [shape for _, shape in arena.requests[:3]] == [(B, T, 4), (B, T, 4, 4), (B, T)]
        assert arena.check() == []


def test_refusals_write_nothing():
    import torch
    from tests import guard_bands as gb
    from chirpgp_amd import _engine as E
    c = cs.chirp_case(T=65)
    s = setup('chirp', 'cd_ekf')
    ys = torch.from_numpy(c.ys.copy()).cuda()
    dts = torch.from_numpy(np.full(65, 1e-3)).cuda()
    lib = E.load_library()
    arena = gb.Arena('cuda', 'aligned')
    with arena.installed():
        out = [arena.output((1, 65, 4), 'mfs'), arena.output((1, 65, 4, 4), 'Pfs'), arena.output((1, 65), 'nll')]
        for dts_ptr, stride, what in ((None, 0, 'dts is NULL'), (E._ptr(dts), -1, 'dts_stride')):
            rc, msg = raw_filter(lib, E, c, E.F_CD_EKF, c.drift, ys, dts_ptr, stride, out)
            assert rc == -1 and what in msg, (rc, msg)
        rc, msg = raw_filter(lib, E, c, E.F_EKF, c.disc, ys, E._ptr(dts), 0, out)
        assert rc == -1 and 'fixed per dt' in msg, (rc, msg)
        with pytest.raises(RuntimeError, match='CGP_RK4_SUBSTEPS'):      # substeps one lane per trial: refused as on the plain entry point
            s.smooth(np.zeros((65, 4)), np.stack([np.eye(4)] * 65), np.full(65, 1e-3), substeps=2, flags=THREAD)
    torch.cuda.synchronize()
    assert arena.written() == [] and arena.guard_violations() == []


# ---- the two entry points through raw ctypes
def raw_filter(lib, E, c, method, spec, ys, dts_ptr, dts_stride, out, B=1, flags=0):
    import torch
    keep = []
    with torch.cuda.device(ys.device):
        ctx = E.context(ys.device.index)
        gamma = c.disp.outer() if method == E.F_CD_EKF else None
        model = E._model_struct(spec, gamma, B, keep)
        init = E._init_struct(c.H, c.Xi, c.m0, c.P0, 4, B, keep)
        T = int(ys.shape[-1])
        rc = lib.cgp_filter_timed(ctx, method, C.byref(model), None, C.byref(init), dts_ptr, dts_stride, E._ptr(ys), T, 1, None, B, T,
                                  E._ptr(out[0]), E._ptr(out[1]), E._ptr(out[2]), flags, E._stream())
        msg = lib.cgp_last_error(ctx)
        return rc, msg.decode() if msg else ''


def test_raw_entry_points():
    import torch
    from chirpgp_amd import _engine as E
    s = setup('chirp', 'cd_ekf')
    c, T = s.c, 130
    want = oracle_filter('chirp', 'cd_ekf', 1)
    lib = E.load_library()
    ys = torch.from_numpy(c.ys.copy()).cuda()
    dts = torch.from_numpy(s.grids[0].copy()).cuda()
    out = [torch.full((1, T, 4), np.nan, dtype=torch.float64, device='cuda'), torch.full((1, T, 4, 4), np.nan, dtype=torch.float64, device='cuda'),
           torch.full((1, T), np.nan, dtype=torch.float64, device='cuda')]
    rc, msg = raw_filter(lib, E, c, E.F_CD_EKF, c.drift, ys, E._ptr(dts), 0, out)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert worst([o.cpu().numpy() for o in out], want, 'cgp_filter_timed, raw') <= GATE
    # empty calls: CGP_OK, nothing touched -- not even a NULL dts is looked at
    rc, msg = raw_filter(lib, E, c, E.F_CD_EKF, c.drift, ys, None, 0, out, B=0)
    assert rc == 0, msg
    # cgp_smoother_timed on those rows, full rows through a cgp_smooth_out
    keep = []
    with torch.cuda.device(ys.device):
        ctx = E.context(ys.device.index)
        model = E._model_struct(c.drift, c.disp.outer(), 1, keep)
        mss, Pss = torch.full_like(out[0], np.nan), torch.full_like(out[1], np.nan)
        o = E.CgpSmoothOut()
        o.mss, o.Pss, o.comp = E._ptr(mss), E._ptr(Pss), -1
        rc = lib.cgp_smoother_timed(ctx, E.S_CD_EKS, C.byref(model), None, E._ptr(dts), 0, 1, None, E._ptr(out[0]), E._ptr(out[1]), 1, T,
                                    C.byref(o), 0, E._stream())
        assert rc == 0, lib.cgp_last_error(ctx)
        torch.cuda.synchronize()
        mf, Pf = out[0].cpu().numpy()[0], out[1].cpu().numpy()[0]
        want_s = s.osmooth(mf, Pf, s.grids[0])
        assert np.isfinite(want_s[0]).all()
        assert worst([mss.cpu().numpy()[0], Pss.cpu().numpy()[0]], want_s, 'cgp_smoother_timed, raw') <= GATE
        for bad, what in (((None, 0, 1), 'dts is NULL'), ((E._ptr(dts), -1, 1), 'dts_stride'), ((E._ptr(dts), 0, 0), 'dts_repeat')):
            rc = lib.cgp_smoother_timed(ctx, E.S_CD_EKS, C.byref(model), None, bad[0], bad[1], bad[2], None, E._ptr(out[0]), E._ptr(out[1]), 1, T,
                                        C.byref(o), 0, E._stream())
            assert rc == -1 and what in lib.cgp_last_error(ctx).decode()


# ---- the MLE objective
def jittered_record(T):
    """A chirp observed at jittered times: sin(2 pi (f0 t + t^2)) + noise at its own time stamps."""
    rng = np.random.default_rng(3)
    dts = to.grid(T, 1e-2, 0.5, seed=5)
    ts = np.cumsum(dts)
    return np.sin(2 * np.pi * (5. * ts + ts ** 2)) + np.sqrt(0.1) * rng.standard_normal(T), dts


def oracle_nll(params, ys, dts, Xi=0.1):
    from oracle import np_filters as onp
    from oracle import np_models as om
    drift, disp, _, m0, P0, H = om.build_chirp_model(params)
    return to.run_filter(onp.cd_ekf, drift, disp, H, Xi, m0, P0, dts, ys)[2][-1]


def test_mle_takes_the_intervals():
    from chirpgp_amd import mle
    from chirpgp_amd import models as pm
    s = setup('chirp', 'cd_ekf')
    ys, dts = s.c.ys, s.grids[0]
    p0 = np.array([0.1, 0.1, 0.1, 1., 1., 7.])
    params = np.stack([p0, p0 * 1.1, p0 * 0.9])
    thetas = pm.g_inv(params)
    want = np.array([oracle_nll(p, ys, dts) for p in pm.g(thetas)])
    assert np.isfinite(want).all()
    got = mle.batched_nll('cd_ekf', pm.build_chirp_model, thetas, ys, 0.1, None, dts=dts)
    assert worst([got], [want], 'batched_nll, jittered chirp') <= GATE
    best, nll, arg = mle.grid_search('cd_ekf', pm.build_chirp_model, params, ys, 0.1, None, dts=dts)
    assert np.array_equal(nll[0], got) and arg[0] == int(np.argmin(want))
    f, grad = mle.make_objective('cd_ekf', pm.build_chirp_model, ys, 0.1, None, dts=dts, missing='skip', substeps=1)(thetas[0])
    assert f == got[0] and np.isfinite(grad).all() and np.abs(grad).max() > 0


def test_fit_on_a_jittered_record():
    """fit('cd_ekf', dts=) on a T = 200 jittered record ends finite and not above where it started; the objective at the optimum is the
    oracle's there."""
    from chirpgp_amd import mle
    from chirpgp_amd import models as pm
    ys, dts = jittered_record(200)
    p0 = so.chirp_params(5.)
    start = mle.batched_nll('cd_ekf', pm.build_chirp_model, pm.g_inv(p0)[None], ys, 0.1, None, dts=dts)[0]
    opt, res = mle.fit('cd_ekf', pm.build_chirp_model, p0, ys, 0.1, None, dts=dts, maxiter=30)
    print(f'fit cd_ekf on the jittered record: NLL {start:.6f} -> {res.fun:.6f} in {res.nfev} launches')
    assert np.isfinite(start) and np.isfinite(res.fun) and res.fun <= start
    want = oracle_nll(opt, ys, dts)
    assert np.isfinite(want) and cs.max_rel_err(np.array([res.fun]), np.array([want])) <= GATE
    many, info = mle.fit_many('cd_ekf', pm.build_chirp_model, p0, np.stack([ys, ys[::-1]]), 0.1, None, dts=np.stack([dts, dts[::-1]]), maxiter=3)
    assert np.isfinite(info['fun']).all()
