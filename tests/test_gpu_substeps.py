"""`substeps=n` (CGP_RK4_SUBSTEPS, include/chirpgp_hip.h) on the GPU: cd_ekf, cd_sgp_filter, cd_eks and cd_sgp_smoother with n RK4 steps of
dt / n between two measurements, against the refined-grid NumPy oracle that defines them (tests/substeps_oracle.py) and against the
engine's own emulation -- the record refined n times, missing='skip', step dt / n, every n-th row.

Shapes: T = 1, 64, 65 and 130 (the ends of the kernels' 64-step chunks; a filter's shorter records are prefixes of the longest, a smoother's
are not and have an oracle of their own), B = 1 and 3 (three different records), n = 2, 3 (dt / 3 is inexact), 4 and 16; one wavefront and
one lane per trial; the d = 4 chirp and La Scala SDE, the three-harmonic SDE at d = 8, a linear SDE and the Lorenz-63 source model at d = 3.  Gate: max_rel_err <= 1e-9,
the project's (tests/test_gpu_gaps.py: GATE).

Every test here fails on the parent commit: the keyword does not exist there (TypeError: run_filter() got an unexpected keyword argument
'substeps'), and the flag bits were ignored by cgp_filter and cgp_smoother.

Largest max_rel_err seen on an MI355X (every case prints its own): filters on the route the call takes and on the forced generic wave
kernel 5.3e-15 (harm3 cd_sgp, n = 2), one lane per trial 1.5e-15; with real gaps 5.1e-15; smoothers 1.5e-15 (linear3 cd_eks, n = 4); against
the gap emulation 1.4e-16 (filters) and 3.0e-16 (smoothers); the 60 Hz record with n = 4 2.5e-15; mle.batched_nll 2.1e-15.  The exact
gradient against 100 digits: value 1.2e-15, gradient 2.7e-15 of its scale (sub_chirp_n3_H); against the float64 tangent oracle on the longer
records: value 8.6e-16, gradient 4.0e-14 (20 Hz, n = 4).  fit(exact=True, substeps=4) on the T = 200 record ended at an NLL of 60.391765017
in 26 launches, the difference route at 60.391765007 in 31: 1.7e-10 relative above it, inside the 1e-6 the test allows.

The Lorenz-63 cases run the model as source, compiled at run time (cgp_filter_custom / cgp_smoother_custom; one launch shape, the launch
flags of the other cases are ignored there)."""
import functools
import math
import os

import numpy as np
import pytest

from tests import cases as cs
from tests import gap_oracle as go
from tests import substeps_oracle as so

pytestmark = pytest.mark.gpu

GATE = 1e-9
WAVE, THREAD, GENERIC = 0x2, 0x4, 0x10
LENGTHS = (1, 64, 65, 130)
SHAPES = ((0, 'default'), (THREAD, 'lane'), (GENERIC | WAVE, 'generic-wave'))


def _fs():
    from chirpgp_amd import filters_smoothers as fs
    return fs


def three_records(ys):
    """Three different records of one length: a batch whose trials cannot be mistaken for one another."""
    rng = np.random.default_rng(7)
    return np.stack([ys, ys + 0.05 * rng.standard_normal(ys.size), ys[::-1].copy()])


class Setup:
    """One (model, method): the engine's filter and smoother, closed over everything but the record, the step and the keywords, and the
    oracle's pair in the oracle's own argument order."""
    def __init__(self, c, method, sg=None):
        from oracle import np_filters as onp
        fs = _fs()
        self.c, self.sig = c, method == 'cd_sgp'
        if self.sig:
            b, ob, head, ohead = c.disp(None), c.o_disp(None), (sg,), (cs.osig(sg),)
            f, s, self.of, self.os = fs.cd_sgp_filter, fs.cd_sgp_smoother, onp.cd_sgp_filter, onp.cd_sgp_smoother
        else:
            b, ob, head, ohead = c.disp, c.o_disp, (), ()
            f, s, self.of, self.os = fs.cd_ekf, fs.cd_eks, onp.cd_ekf, onp.cd_eks
        self.run = lambda ys, dt=c.dt, **kw: f(c.drift, b, *head, c.H, c.Xi, c.m0, c.P0, dt, ys, **kw)
        self.smooth = lambda mf, Pf, dt=c.dt, **kw: s(c.drift, b, *head, mf, Pf, dt, **kw)
        self.ofilter = lambda n, ys: so.run_filter(self.of, n, c.o_drift, ob, *ohead, c.H, c.Xi, c.m0, c.P0, c.dt, ys)
        self.osmooth = lambda n, mf, Pf: so.run_smoother(self.os, n, c.o_drift, ob, *ohead, mf, Pf, c.dt)


@functools.lru_cache(maxsize=None)
def setup(model, method):
    from chirpgp_amd.quadratures import SigmaPoints
    if model == 'chirp':
        return Setup(cs.chirp_case(T=130), method, SigmaPoints.cubature(4))
    if model == 'chirp-gh3':
        return Setup(cs.chirp_case(T=65), method, SigmaPoints.gauss_hermite(4, 3))
    if model == 'lascala':
        return Setup(cs.lascala_case(T=130), method, SigmaPoints.cubature(4))
    if model == 'harm3':
        c = cs.harmonic_case(nh=3, T=65)
        return Setup(c, method, c.sgps)
    if model == 'linear3':
        c = cs.linear_case(0, T=65)
        return Setup(c, method, SigmaPoints.cubature(3))
    if model == 'lorenz':                                  # Lorenz-63 as source, compiled at run time (tests/test_gpu_custom.py)
        from chirpgp_amd import models as pm
        from tests.test_gpu_custom import LORENZ, KAPPA, LAM, MU, lorenz_host, lorenz_data
        drift, _ = lorenz_host()
        sde, disp = pm.custom_sde(LORENZ, 3, np.array([KAPPA, LAM, MU, 25.]), 5. * np.eye(3), host=drift)
        c = cs.Case('lorenz_T65', d=3, dt=1e-3, H=np.array([1., 0., 0.]), Xi=2., m0=np.zeros(3), P0=np.eye(3), ys=lorenz_data(65, 1e-3, 2.),
                    drift=sde, disp=disp, o_drift=drift, o_disp=lambda _: 5. * np.eye(3))
        return Setup(c, method, SigmaPoints.cubature(3))
    raise ValueError(model)


@functools.lru_cache(maxsize=None)
def oracle_filter(model, method, n, B):
    """The refined-grid oracle on the first B of the three records: (kept rows, all n T rows), computed once and never written to."""
    s = setup(model, method)
    rows = [s.ofilter(n, y) for y in three_records(s.c.ys)[:B]]
    out = tuple(tuple(np.stack([r[k][i] for r in rows]) for i in range(3)) for k in range(2))
    for part in out:
        for a in part:
            a.setflags(write=False)
    return out


def worst(got, want, what):
    errs = [cs.max_rel_err(g, w) for g, w in zip(got, want)]
    print(f'{what}: max_rel_err {max(errs):.2e}')
    return max(errs)


# ---- filters against the oracle: every length, both launch shapes, the route the call would take unflagged and the forced generic one
FILTER_CASES = [('chirp', 'cd_ekf', 2, 1), ('chirp', 'cd_ekf', 3, 3), ('chirp', 'cd_ekf', 4, 1), ('chirp', 'cd_ekf', 16, 1),
                ('chirp', 'cd_sgp', 2, 1), ('chirp', 'cd_sgp', 3, 3), ('chirp', 'cd_sgp', 4, 1), ('chirp', 'cd_sgp', 16, 1),
                ('chirp-gh3', 'cd_sgp', 2, 1), ('lascala', 'cd_ekf', 4, 3), ('lascala', 'cd_sgp', 3, 1),
                ('harm3', 'cd_ekf', 3, 3), ('harm3', 'cd_sgp', 2, 1), ('linear3', 'cd_ekf', 4, 3), ('linear3', 'cd_sgp', 3, 1),
                ('lorenz', 'cd_ekf', 3, 3), ('lorenz', 'cd_ekf', 16, 1), ('lorenz', 'cd_sgp', 2, 3)]


@pytest.mark.parametrize('model,method,n,B', FILTER_CASES, ids=[f'{m}-{f}-n{n}-b{B}' for m, f, n, B in FILTER_CASES])
def test_filter_parity(model, method, n, B):
    s = setup(model, method)
    want = oracle_filter(model, method, n, B)[0]
    assert np.isfinite(want[2]).all()
    ys = three_records(s.c.ys)[:B]
    for T in (t for t in LENGTHS if t <= ys.shape[1]):
        for flags, shape in SHAPES:
            got = s.run(ys[:, :T], substeps=n, flags=flags)
            err = worst(got, [w[:, :T] for w in want], f'{model} {method} n={n} B={B} T={T} {shape}')
            assert err <= GATE, (T, shape, err)


def test_one_substep_is_the_plain_call():
    """substeps=1 sets no bit: the same call, the same kernel, the same bits."""
    for method in ('cd_ekf', 'cd_sgp'):
        s = setup('chirp', method)
        for a, b in zip(s.run(s.c.ys, substeps=1), s.run(s.c.ys)):
            assert np.array_equal(a, b, equal_nan=True)
        mf, Pf, _ = s.run(s.c.ys)
        for a, b in zip(s.smooth(mf, Pf, substeps=1), s.smooth(mf, Pf)):
            assert np.array_equal(a, b, equal_nan=True)


# ---- the engine's own emulation: the refined record with gaps at the inserted times
@pytest.mark.parametrize('method', ['cd_ekf', 'cd_sgp'])
@pytest.mark.parametrize('n', [3, 4])
def test_filter_against_the_gap_emulation(method, n):
    s = setup('chirp', method)
    ys = three_records(s.c.ys)[:, :65]
    want, full = so.gap_emulation(s.run, n, ys, s.c.dt)
    got = s.run(ys, substeps=n)
    assert worst(got, want, f'{method} n={n} against the gap emulation') <= GATE
    # ... and the smoother on all n T rows of the emulation, every n-th row kept
    want_s = tuple(a[:, so.kept(n)] for a in s.smooth(full[0], full[1], s.c.dt / n))
    got_s = s.smooth(got[0], got[1], substeps=n)
    assert worst(got_s, want_s, f'{method} smoother n={n} against the gap emulation') <= GATE


# ---- real gaps on top
@pytest.mark.parametrize('method,n,flags', [('cd_ekf', 2, 0), ('cd_ekf', 3, THREAD), ('cd_sgp', 4, 0), ('cd_sgp', 2, THREAD)])
def test_filter_with_real_gaps(method, n, flags):
    s = setup('chirp', method)
    spans = ((0, 1), (5, 12), (63, 65), (120, 130))
    ys = np.stack([go.with_gaps(s.c.ys, spans), s.c.ys, go.with_gaps(s.c.ys, spans, 3)])
    rows = [s.ofilter(n, y)[0] for y in ys]
    want = tuple(np.stack([r[i] for r in rows]) for i in range(3))
    got = s.run(ys, substeps=n, missing='skip', flags=flags)
    assert worst(got, want, f'{method} n={n} with real gaps') <= GATE
    gap = np.isnan(ys)
    prev = np.concatenate([np.zeros((3, 1)), got[2][:, :-1]], axis=1)
    assert np.array_equal(got[2][gap], prev[gap])          # the cumulative NLL holds over a gap


# ---- smoothers against the oracle
SMOOTHER_CASES = [('chirp', 'cd_ekf', 2, 65, 1), ('chirp', 'cd_ekf', 3, 65, 3), ('chirp', 'cd_ekf', 4, 130, 1), ('chirp', 'cd_ekf', 16, 64, 1),
                  ('chirp', 'cd_ekf', 3, 1, 3), ('chirp', 'cd_ekf', 3, 2, 3), ('chirp', 'cd_sgp', 3, 65, 3), ('chirp', 'cd_sgp', 16, 2, 1),
                  ('chirp-gh3', 'cd_sgp', 2, 65, 1), ('lascala', 'cd_ekf', 4, 65, 1), ('harm3', 'cd_ekf', 2, 65, 3), ('harm3', 'cd_sgp', 3, 33, 1),
                  ('linear3', 'cd_ekf', 4, 65, 3), ('linear3', 'cd_sgp', 2, 65, 1),
                  ('lorenz', 'cd_ekf', 3, 65, 3), ('lorenz', 'cd_ekf', 16, 2, 1), ('lorenz', 'cd_sgp', 2, 65, 3), ('lorenz', 'cd_sgp', 2, 1, 3)]


@pytest.mark.parametrize('model,method,n,T,B', SMOOTHER_CASES, ids=[f'{m}-{f}-n{n}-T{T}-b{B}' for m, f, n, T, B in SMOOTHER_CASES])
def test_smoother_parity(model, method, n, T, B):
    """The smoother is given the ORACLE's filtering rows (the kept ones), so that its error is its own."""
    s = setup(model, method)
    kept, full = oracle_filter(model, method, n, B)
    rows = [s.osmooth(n, full[0][b][:n * T], full[1][b][:n * T]) for b in range(B)]
    want = tuple(np.stack([r[i] for r in rows]) for i in range(2))
    assert np.isfinite(want[0]).all()
    mf, Pf = np.ascontiguousarray(kept[0][:, :T]), np.ascontiguousarray(kept[1][:, :T])
    for flags, shape in ((0, 'default'), (GENERIC, 'generic')):
        got = s.smooth(mf, Pf, substeps=n, flags=flags)
        assert worst(got, want, f'{model} {method} smoother n={n} T={T} B={B} {shape}') <= GATE


def test_smoother_runs_one_wavefront_per_trial_whatever_the_batch():
    """B = 70 crosses a 64-trial block of the one-lane-per-trial shape, which a flagged smoother never takes; asking for it is refused."""
    s = setup('chirp', 'cd_ekf')
    kept, full = oracle_filter('chirp', 'cd_ekf', 3, 3)
    want = tuple(np.stack([r[i] for r in [s.osmooth(3, full[0][b][:3 * 64], full[1][b][:3 * 64]) for b in range(3)]]) for i in range(2))
    idx = np.arange(70) % 3
    got = s.smooth(np.ascontiguousarray(kept[0][idx, :64]), np.ascontiguousarray(kept[1][idx, :64]), substeps=3)
    assert worst(got, [w[idx] for w in want], 'cd_eks n=3 B=70') <= GATE
    with pytest.raises(RuntimeError, match='CGP_RK4_SUBSTEPS'):
        s.smooth(kept[0][:, :64], kept[1][:, :64], substeps=3, flags=THREAD)


# ---- select= forms
@pytest.mark.parametrize('method', ['cd_ekf', 'cd_sgp'])
def test_select_forms(method):
    s = setup('chirp', method)
    kept, _ = oracle_filter('chirp', method, 3, 3)
    mf, Pf = np.ascontiguousarray(kept[0][:, :65]), np.ascontiguousarray(kept[1][:, :65])
    mss, Pss = s.smooth(mf, Pf, substeps=3)
    sel = dict(comp=2, mean=True, var=True, expect='softplus', order=10)
    m2, P2, picked = s.smooth(mf, Pf, substeps=3, select=sel)
    assert np.array_equal(m2, mss) and np.array_equal(P2, Pss)
    assert np.array_equal(picked.mean, mss[..., 2]) and np.array_equal(picked.var, Pss[..., 2, 2])
    none_m, none_P, alone = s.smooth(mf, Pf, substeps=3, select=sel, want=(False, False))      # (rows of its own behind the scenes)
    assert none_m is None and none_P is None
    assert all(np.array_equal(alone[k], picked[k]) for k in ('mean', 'var', 'expect'))
    plain = s.smooth(mf, Pf, select=sel)[2]
    assert not np.array_equal(plain.mean, picked.mean)      # the count reached the kernel


# ---- stores: every row of every output, nothing else
@pytest.mark.parametrize('T,B,flags', [(1, 1, 0), (65, 3, 0), (130, 3, THREAD), (64, 70, THREAD)])
def test_stores(T, B, flags):
    import torch
    from tests import guard_bands as gb
    for method in ('cd_ekf', 'cd_sgp'):
        s = setup('chirp', method)
        ys = torch.from_numpy(three_records(s.c.ys)[np.arange(B) % 3, :T].copy()).cuda()
        arena = gb.Arena('cuda', 'aligned')
        with arena.installed():
            mf, Pf, nll = s.run(ys, substeps=3, flags=flags)
            if not flags:
                s.smooth(mf, Pf, substeps=3)
        assert [shape for _, shape in arena.requests[:3]] == [(B, T, 4), (B, T, 4, 4), (B, T)]
        assert arena.check() == []


# ---- instability rescued
def test_instability_rescued():
    """2 pi f dt = 3.77: one RK4 step per sample ends in NaN on the engine as on the oracle, four are finite and the oracle's."""
    from chirpgp_amd import models as pm
    from oracle import np_filters as onp
    fs = _fs()
    ys = so.chirp_record(60.)
    drift, disp, _, m0, P0, H = pm.build_chirp_model(so.chirp_params(60.))
    odrift, odisp, _, om0, oP0, oH = so.chirp_model(60.)
    for flags in (0, THREAD):
        one = fs.cd_ekf(drift, disp, H, 0.1, m0, P0, 1e-2, ys, substeps=1, flags=flags)
        assert math.isnan(one[2][-1])
        assert math.isnan(onp.cd_ekf(odrift, odisp, oH, 0.1, om0, oP0, 1e-2, ys)[2][-1])
        four = fs.cd_ekf(drift, disp, H, 0.1, m0, P0, 1e-2, ys, substeps=4, flags=flags)
        want, _ = so.run_filter(onp.cd_ekf, 4, odrift, odisp, oH, 0.1, om0, oP0, 1e-2, ys)
        assert math.isfinite(four[2][-1]) and round(float(want[2][-1]), 1) == 375.4
        assert worst(four, want, '60 Hz, n=4') <= GATE


# ---- the MLE objective
def test_mle_objective_takes_the_substeps():
    """batched_nll, make_objective, grid_search and fit with substeps=4 on the 60 Hz record, where one step per sample gives no likelihood at
    all: the oracle's NLL at three parameter vectors, a difference gradient of that objective, a search that goes downhill from 375.4."""
    from chirpgp_amd import mle
    from chirpgp_amd import models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    from oracle import np_filters as onp
    from oracle import np_models as om
    ys = so.chirp_record(60.)
    p0 = so.chirp_params(60.)
    thetas = pm.g_inv(np.stack([p0, p0 * 1.1, p0 * 0.9]))
    assert np.isnan(mle.batched_nll('cd_ekf', pm.build_chirp_model, thetas, ys, 0.1, 1e-2)).all()
    want = []
    for p in pm.g(thetas):
        drift, disp, _, m0, P0, H = om.build_chirp_model(p)
        want.append(so.run_filter(onp.cd_ekf, 4, drift, disp, H, 0.1, m0, P0, 1e-2, ys)[0][2][-1])
    got = mle.batched_nll('cd_ekf', pm.build_chirp_model, thetas, ys, 0.1, 1e-2, substeps=4)
    assert worst([got], [np.array(want)], 'batched_nll cd_ekf n=4') <= GATE and round(float(got[0]), 1) == 375.4
    sg = SigmaPoints.cubature(4)
    got_s = mle.batched_nll('cd_sgp_filter', pm.build_chirp_model, thetas, ys, 0.1, 1e-2, sgps=sg, substeps=8)
    want_s = []
    for p in pm.g(thetas):
        drift, disp, _, m0, P0, H = om.build_chirp_model(p)
        want_s.append(so.run_filter(onp.cd_sgp_filter, 8, drift, disp(None), cs.osig(sg), H, 0.1, m0, P0, 1e-2, ys)[0][2][-1])
    assert np.isfinite(want_s).all() and worst([got_s], [np.array(want_s)], 'batched_nll cd_sgp_filter n=8') <= GATE
    f, grad = mle.make_objective('cd_ekf', pm.build_chirp_model, ys, 0.1, 1e-2, substeps=4)(thetas[0])
    assert f == got[0] and np.isfinite(grad).all() and np.abs(grad).max() > 0
    best, nll, arg = mle.grid_search('cd_ekf', pm.build_chirp_model, pm.g(thetas), ys, 0.1, 1e-2, substeps=4)
    assert np.array_equal(nll[0], got) and arg[0] == int(np.argmin(got))


# ---- the exact gradient: cgp_cd_ekf_nll_grad with the flag, against 100-digit arithmetic and the float64 tangent oracle
SUB_Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'exact_cd_substeps.npz'))
SUB_NAMES = [str(n) for n in SUB_Z['names']]


def sub_case(name):
    """A case of tests/golden/exact_cd_substeps.npz in the form tests/cd_grad_cases.py's helpers take."""
    c = {k: SUB_Z[f'{name}.{k}'] for k in ('theta', 'ys', 'H', 'grad')}
    c.update({k: float(SUB_Z[f'{name}.{k}']) for k in ('Xi', 'dt', 'nll', 'moved_nll', 'moved_grad')})
    c.update(name=name, build=str(SUB_Z[f'{name}.build']), n=int(SUB_Z[f'{name}.n']), skip=int(SUB_Z[f'{name}.skip']), with_dxi=0)
    return c


@pytest.mark.parametrize('name', SUB_NAMES)
def test_gradient_against_100_digits(name):
    """Every fixture case through the raw C-ABI (with CGP_SKIP_MISSING as well where the record has gaps of its own) and through
    mle.value_and_grad, at the gates of tests/cd_grad_cases.py: value 1e-11 relative, gradient 1e-8 of its scale."""
    from chirpgp_amd import _engine as E, mle
    from tests import cd_grad_cases as cg
    c = sub_case(name)
    assert c['moved_nll'] < cg.VALUE_MOVE_MAX and c['moved_grad'] < cg.GRAD_MOVE_MAX and 2 <= c['n'] <= 4 and len(c['ys']) <= 40
    flags = E.rk4_substeps(c['n']) | (cg.SKIP_MISSING if c['skip'] else 0)
    rc, msg, nll, grad = cg.raw(c, len(c['ys']), cg.directions(c)[0], flags=flags)
    assert rc == 0, msg
    ev, eg = cg.errors(nll[0], grad[0], c['nll'], c['grad'], f'{name} (n = {c["n"]}), C-ABI')
    assert ev <= cg.VALUE_RTOL and eg <= cg.GRAD_GATE
    if np.array_equal(c['H'], [0., 1., 0., 0.]):           # (mle takes the builder's H)
        f, g_ = mle.value_and_grad(cg.builder(c['build']), c['theta'][None, :], c['ys'], c['Xi'], c['dt'], method='cd_ekf', substeps=c['n'],
                                   missing='skip' if c['skip'] else None)
        ev, eg = cg.errors(f[0], g_[0], c['nll'], c['grad'], f'{name} (n = {c["n"]}), mle.value_and_grad')
        assert ev <= cg.VALUE_RTOL and eg <= cg.GRAD_GATE
    # without the flag the same call answers another question: the count reached the kernel
    rc, msg, nll1, grad1 = cg.raw(c, len(c['ys']), cg.directions(c)[0], flags=flags & cg.SKIP_MISSING)
    assert rc == 0 and nll1[0] != nll[0] and not np.array_equal(grad1[0], grad[0])


@pytest.mark.parametrize('which', ['coarse-20Hz', 'gapped-chirp'])
def test_gradient_on_longer_records(which):
    """Two longer records against the float64 tangent oracle (tests/cd_grad_oracle.py on the refined record), same gates: the 20 Hz record
    of 150 samples at dt = 1e-2 with n = 4, and 262 samples at dt = 1e-3 with gaps of their own and n = 3; three parameter vectors each."""
    from chirpgp_amd import mle
    from chirpgp_amd import models as pm
    from tests import cd_grad_cases as cg
    if which == 'coarse-20Hz':
        ys, dt, n, missing, p0 = so.chirp_record(20.), 1e-2, 4, None, so.chirp_params(20.)
    else:
        c = cs.chirp_case(T=262)
        ys, dt, n, missing, p0 = go.with_gaps(c.ys, ((0, 1), (5, 12), (63, 65), (128, 192), (250, 262))), c.dt, 3, 'skip', np.array([0.1, 0.1, 0.1, 1., 1., 7.])
    thetas = pm.g_inv(np.stack([p0, p0 * 1.1, p0 * 0.9]))
    f, g_ = mle.value_and_grad(pm.build_chirp_model, thetas, ys, 0.1, dt, method='cd_ekf', substeps=n, missing=missing)
    for i, th in enumerate(thetas):
        want_f, want_g = so.value_and_grad('chirp', th, ys, 0.1, dt, n)
        assert np.isfinite(want_f) and np.isfinite(want_g).all()
        ev, eg = cg.errors(f[i], g_[i], want_f, want_g, f'{which} n = {n}, theta {i}')
        assert ev <= cg.VALUE_RTOL and eg <= cg.GRAD_GATE


def test_fit_with_the_exact_gradient():
    """fit(method='cd_ekf', exact=True, substeps=4) on a T = 200 record (20 Hz at dt = 1e-2) ends at an NLL no higher than the difference
    route's plus 1e-6 relative."""
    from chirpgp_amd import mle
    from chirpgp_amd import models as pm
    ys, p0 = so.chirp_record(20., T=200), so.chirp_params(20.)
    _, exact = mle.fit('cd_ekf', pm.build_chirp_model, p0, ys, 0.1, 1e-2, exact=True, substeps=4)
    _, diff = mle.fit('cd_ekf', pm.build_chirp_model, p0, ys, 0.1, 1e-2, exact=False, substeps=4)
    print(f'fit cd_ekf n=4, T=200: exact NLL {exact.fun:.9f} ({exact.nfev} launches), differences {diff.fun:.9f} ({diff.nfev} launches)')
    assert np.isfinite(exact.fun) and np.isfinite(diff.fun)
    assert exact.fun <= diff.fun + 1e-6 * abs(diff.fun)


# ---- what is refused, on the device: the call returns its code and writes nothing
def test_refusals_write_nothing():
    import torch
    from tests import guard_bands as gb
    from chirpgp_amd import _engine as E
    fs = _fs()
    c = cs.chirp_case(T=65)
    ys = torch.from_numpy(c.ys.copy()).cuda()
    arena = gb.Arena('cuda', 'aligned')
    with arena.installed():
        with pytest.raises(RuntimeError, match='CGP_RK4_SUBSTEPS'):
            fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, ys, flags=E.rk4_substeps(2))             # a discrete method, past the Python check
        with pytest.raises(RuntimeError, match='CGP_RK4_SUBSTEPS'):
            fs.cd_ekf(c.drift, c.disp, c.H, c.Xi, c.m0, c.P0, c.dt, ys, flags=E.rk4_substeps(2), time_split=(2, 0))
    torch.cuda.synchronize()
    assert arena.written() == [] and arena.guard_violations() == []
