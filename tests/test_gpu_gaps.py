"""missing='skip' (CGP_SKIP_MISSING) on the GPU: records with NaN gaps through every filter, against the gapped NumPy oracle
(tests/gap_oracle.py), and the identities the flag promises -- see include/chirpgp_hip.h, cgp_filter.

The record: the demos' chirp model (cases.chirp_case(T=262), Xi = 0.1), missing at step 0, steps 5-11, 63-64 (across a chunk boundary),
128-191 (one whole 64-step chunk) and 250-261 (a forecast tail, the last step included); T = 262 leaves 6 steps behind four chunks.  The
batch: that record, the record without gaps, a record of NaN only, and the pattern moved by 1 and by 3 steps -- B = 5, so that no gap
decision is uniform across the trials of a wavefront in the one-lane-per-trial shape; B = 70 repeats the five across one 64-trial block.

Gate against the oracle: max_rel_err <= 1e-9 (the project's own; the oracle's response to a 1e-15 relative perturbation
of the measurements is at most 2.2e-13 of an output's scale on this record).  Worst values measured on an MI355X: docs/KERNELS.md."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cases as cs
from tests import gap_oracle as go

pytestmark = pytest.mark.gpu

GATE = 1e-9
WAVE, THREAD, GENERIC, SKIP = 0x2, 0x4, 0x10, 0x2000
SPANS = ((0, 1), (5, 12), (63, 65), (128, 192), (250, 262))          # T = 262
SPANS_140 = ((0, 1), (5, 12), (63, 65), (70, 90), (130, 140))        # the T = 140 records of the d = 8, KPT and run-time compiled models
MIX = np.array([0.3, 1.0, -0.2, 0.1])                                # a measurement vector that is not e_1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fs():
    from chirpgp_amd import filters_smoothers as fs
    return fs


def records(ys, spans):
    """The batch of five: gapped | whole | NaN only | the pattern moved by 1 | by 3."""
    return np.stack([go.with_gaps(ys, spans), np.array(ys), np.full_like(ys, np.nan), go.with_gaps(ys, spans, 1), go.with_gaps(ys, spans, 3)])


class Setup:
    """One (model, method): `run(ys, **kw)` on the engine, `oracle(ys_row)` on the gapped NumPy oracle, `smooth` / `osmooth` behind them."""
    def __init__(self, name, T, spans, ys, run, oracle, smooth=None, osmooth=None, same_kernel_flags=None):
        self.name, self.T, self.spans, self.ys = name, T, spans, ys
        self.run, self.oracle, self.smooth, self.osmooth = run, oracle, smooth, osmooth
        self.same_kernel_flags = same_kernel_flags        # launches where the flagged and the unflagged call take the same kernel


def _lorenz():
    from tests.test_gpu_custom import LORENZ, KAPPA, LAM, MU, lorenz_host, lorenz_data
    from chirpgp_amd import models as pm
    drift, m_and_cov = lorenz_host()
    p = np.array([KAPPA, LAM, MU, 25.])
    return pm.custom_cond_m_cov(LORENZ, 3, p, host=m_and_cov), m_and_cov, lorenz_data(140, 1e-3, 2.)


@functools.lru_cache(maxsize=None)
def setups():
    from chirpgp_amd.quadratures import SigmaPoints
    from oracle import np_filters as onp
    fs = _fs()
    out = {}

    def add(s):
        out[s.name] = s

    for model, c in (('chirp', cs.chirp_case(T=262)), ('lascala', cs.lascala_case(T=262))):
        for hname, H in (('e1', c.H), ('mix', MIX)):
            if model == 'lascala' and hname == 'mix':
                continue
            sets = (('gh3', c.sgps), ('cub', SigmaPoints.cubature(4))) if model == 'chirp' else (('gh3', c.sgps),)
            add(Setup(f'ekf-{model}-{hname}', 262, SPANS, c.ys,
                      lambda ys, c=c, H=H, m0=None, P0=None, **kw: fs.ekf(c.disc, H, c.Xi, c.m0 if m0 is None else m0, c.P0 if P0 is None else P0, c.dt, ys, **kw),
                      lambda y, c=c, H=H: go.gapped(onp.ekf, c.o_disc, H, c.Xi, c.m0, c.P0, c.dt, y),
                      lambda mf, Pf, c=c: fs.eks(c.disc, mf, Pf, c.dt), lambda mf, Pf, c=c: onp.eks(c.o_disc, mf, Pf, c.dt),
                      same_kernel_flags=(GENERIC, GENERIC | WAVE, GENERIC | THREAD)))
            for sname, sg in sets:
                add(Setup(f'sgp_{sname}-{model}-{hname}', 262, SPANS, c.ys,
                          lambda ys, c=c, H=H, sg=sg, m0=None, P0=None, **kw: fs.sgp_filter(c.disc, sg, H, c.Xi, c.m0 if m0 is None else m0, c.P0 if P0 is None else P0, c.dt, ys, **kw),
                          lambda y, c=c, H=H, sg=sg: go.gapped(onp.sgp_filter, c.o_disc, cs.osig(sg), H, c.Xi, c.m0, c.P0, c.dt, y),
                          lambda mf, Pf, c=c, sg=sg: fs.sgp_smoother(c.disc, sg, mf, Pf, c.dt),
                          lambda mf, Pf, c=c, sg=sg: onp.sgp_smoother(c.o_disc, cs.osig(sg), mf, Pf, c.dt),
                          same_kernel_flags=(0, WAVE, GENERIC, GENERIC | THREAD)))
            if model == 'chirp':
                add(Setup(f'cd_ekf-chirp-{hname}', 262, SPANS, c.ys,
                          lambda ys, c=c, H=H, m0=None, P0=None, **kw: fs.cd_ekf(c.drift, c.disp, H, c.Xi, c.m0 if m0 is None else m0, c.P0 if P0 is None else P0, c.dt, ys, **kw),
                          lambda y, c=c, H=H: go.gapped(onp.cd_ekf, c.o_drift, c.o_disp, H, c.Xi, c.m0, c.P0, c.dt, y),
                          lambda mf, Pf, c=c: fs.cd_eks(c.drift, c.disp, mf, Pf, c.dt), lambda mf, Pf, c=c: onp.cd_eks(c.o_drift, c.o_disp, mf, Pf, c.dt),
                          same_kernel_flags=(0, WAVE, GENERIC, GENERIC | THREAD)))
                add(Setup(f'cd_sgp-chirp-{hname}', 262, SPANS, c.ys,
                          lambda ys, c=c, H=H, m0=None, P0=None, **kw: fs.cd_sgp_filter(c.drift, c.disp(None), c.sgps, H, c.Xi, c.m0 if m0 is None else m0, c.P0 if P0 is None else P0, c.dt, ys, **kw),
                          lambda y, c=c, H=H: go.gapped(onp.cd_sgp_filter, c.o_drift, c.o_disp(None), cs.osig(c.sgps), H, c.Xi, c.m0, c.P0, c.dt, y),
                          lambda mf, Pf, c=c: fs.cd_sgp_smoother(c.drift, c.disp(None), c.sgps, mf, Pf, c.dt),
                          lambda mf, Pf, c=c: onp.cd_sgp_smoother(c.o_drift, c.o_disp(None), cs.osig(c.sgps), mf, Pf, c.dt),
                          same_kernel_flags=(0, WAVE, GENERIC, GENERIC | THREAD)))
    li = cs.linear_case(0, T=262)
    add(Setup('kf-linear3', 262, SPANS, li.ys,
              lambda ys, m0=None, P0=None, **kw: fs.kf(li.F, li.Sigma, li.H, li.Xi, li.m0 if m0 is None else m0, li.P0 if P0 is None else P0, ys, **kw),
              lambda y: go.gapped(onp.kf, li.F, li.Sigma, li.H, li.Xi, li.m0, li.P0, y), same_kernel_flags=(0, WAVE, THREAD)))
    h = cs.harmonic_case(nh=3, T=140)
    add(Setup('ekf-harm3', 140, SPANS_140, h.ys, lambda ys, **kw: fs.ekf(h.disc, h.H, h.Xi, h.m0, h.P0, h.dt, ys, **kw),
              lambda y: go.gapped(onp.ekf, h.o_disc, h.H, h.Xi, h.m0, h.P0, h.dt, y), same_kernel_flags=(GENERIC, GENERIC | THREAD)))
    add(Setup('sgp-harm3', 140, SPANS_140, h.ys, lambda ys, **kw: fs.sgp_filter(h.disc, h.sgps, h.H, h.Xi, h.m0, h.P0, h.dt, ys, **kw),
              lambda y: go.gapped(onp.sgp_filter, h.o_disc, cs.osig(h.sgps), h.H, h.Xi, h.m0, h.P0, h.dt, y), same_kernel_flags=(GENERIC, GENERIC | THREAD)))
    k = cs.kpt_case(T=140)
    add(Setup('kpt2', 140, SPANS_140, k.ys, lambda ys, **kw: fs.ekf_for_kpt(k.F, k.Sigma, k.h, k.Xi, k.m0, k.P0, k.dt, ys, **kw),
              lambda y: go.gapped_ekf_for_kpt(k.F, k.Sigma, k.o_h, k.Xi, k.m0, k.P0, k.dt, y), same_kernel_flags=(GENERIC, GENERIC | THREAD)))
    disc, m_and_cov, lys = _lorenz()
    H3, m03, P03 = np.array([1., 0., 0.]), np.zeros(3), np.eye(3)
    add(Setup('ekf-lorenz-custom', 140, SPANS_140, lys, lambda ys, **kw: fs.ekf(disc, H3, 2., m03, P03, 1e-3, ys, **kw),
              lambda y: go.gapped(onp.ekf, m_and_cov, H3, 2., m03, P03, 1e-3, y), same_kernel_flags=(0,)))
    sg3 = SigmaPoints.cubature(3)
    add(Setup('sgp-lorenz-custom', 140, SPANS_140, lys, lambda ys, **kw: fs.sgp_filter(disc, sg3, H3, 2., m03, P03, 1e-3, ys, **kw),
              lambda y: go.gapped(onp.sgp_filter, m_and_cov, cs.osig(sg3), H3, 2., m03, P03, 1e-3, y), same_kernel_flags=(0,)))
    return out


NAMES = ['ekf-chirp-e1', 'ekf-chirp-mix', 'sgp_gh3-chirp-e1', 'sgp_gh3-chirp-mix', 'sgp_cub-chirp-e1', 'sgp_cub-chirp-mix', 'cd_ekf-chirp-e1',
         'cd_ekf-chirp-mix', 'cd_sgp-chirp-e1', 'cd_sgp-chirp-mix', 'ekf-lascala-e1', 'sgp_gh3-lascala-e1', 'kf-linear3', 'ekf-harm3', 'sgp-harm3',
         'kpt2', 'ekf-lorenz-custom', 'sgp-lorenz-custom']
CUSTOM = ('ekf-lorenz-custom', 'sgp-lorenz-custom')
# launch shapes: (flags, B); a run-time compiled model has one shape and takes no launch flags
SHAPES = [(0, 5, 'default'), (WAVE, 5, 'wave'), (THREAD, 5, 'lane'), (THREAD, 70, 'lane-b70'), (GENERIC, 5, 'generic'), (GENERIC | WAVE, 70, 'generic-wave-b70')]


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    """The gapped oracle on the five records of a setup: computed once, shared by every test, never written to."""
    s = setups()[name]
    rows = [s.oracle(y) for y in records(s.ys, s.spans)]
    out = tuple(np.stack([r[i] for r in rows]) for i in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def batch_of(s, B):
    five = records(s.ys, s.spans)
    return five[np.arange(B) % 5]


def check_identities(s, ys, nll, mfs, Pfs):
    """What the flag promises of any flagged launch, whatever the kernel."""
    prev = np.concatenate([np.zeros((nll.shape[0], 1)), nll[:, :-1]], axis=1)
    gap = np.isnan(ys)
    assert np.array_equal(nll[gap], prev[gap]), f'{s.name}: the cumulative NLL moves at a missing step'
    allnan = gap.all(axis=1)
    assert allnan.any()
    assert np.all(nll[allnan] == 0.0) and not np.signbit(nll[allnan]).any(), f'{s.name}: NLL of a record of NaN only'
    assert np.isfinite(mfs[allnan]).all() and np.isfinite(Pfs[allnan]).all(), f'{s.name}: a pure forecast is finite'


ORACLE_CASES = [pytest.param(n, f, B, id=f'{n}-{i}') for n in NAMES if n not in CUSTOM for f, B, i in SHAPES] + \
               [pytest.param(n, 0, B, id=f'{n}-b{B}') for n in CUSTOM for B in (5, 70)]


@pytest.mark.parametrize('name, flags, B', ORACLE_CASES)
def test_against_the_gapped_oracle(name, flags, B):
    s = setups()[name]
    ys = batch_of(s, B)
    mfs, Pfs, nll = s.run(ys, flags=flags, missing='skip')
    want = oracle_rows(name)
    worst = {}
    for g, w, what in zip((mfs, Pfs, nll), want, ('mfs', 'Pfs', 'nll')):
        worst[what] = max(cs.max_rel_err(g[b], w[b % 5]) for b in range(B))
    print(f'{name} flags={flags:#x} B={B}: ' + ' '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    for what, e in worst.items():
        assert e <= GATE, (name, what, e)
    check_identities(s, ys, nll, mfs, Pfs)
    # a trial's rows do not depend on which other trials share its launch
    for b in range(5, B):
        for g in (mfs, Pfs, nll):
            assert np.array_equal(g[b], g[b % 5]), (name, b)


@pytest.mark.parametrize('name', ['ekf-chirp-e1', 'sgp_gh3-chirp-e1', 'cd_ekf-chirp-mix', 'kpt2'])
def test_final_nll_only(name):
    s = setups()[name]
    ys = batch_of(s, 5)
    for flags in (0, THREAD, GENERIC):
        _, _, nll = s.run(ys, flags=flags, missing='skip', nll_final_only=True, want=(False, False, True))
        want = oracle_rows(name)[2][:, -1]
        assert nll.shape == (5,)
        assert nll[2] == 0.0
        assert cs.max_rel_err(nll, want) <= GATE, (name, flags, cs.max_rel_err(nll, want))


@pytest.mark.parametrize('name', NAMES)
def test_flag_changes_nothing_on_a_record_without_gaps(name):
    """Flagged and unflagged launches that take the same kernel agree bit for bit on the NaN-free trial -- alone in its launch and among
    the records with gaps.

    One class of launches cannot promise the second, with or without the flag: the sigma-point filters with one lane per trial.  There the
    WAVEFRONT chooses the tier of the fan's softplus -> sin / cos chain for all its lanes (cgp_steps.hpp: sgp4_prediction_collapsed and its
    kin -- lean, branch-free full accuracy, checked), so a trial whose neighbour leaves the lean regime (a pure forecast does) is evaluated
    by another tier of the same functions.  The tiers agree to their accuracy, 7e-12 of the rotation angle at worst (cgp_fastmath.hpp), which
    is what the 1e-9 gate against the oracle already allows; that gate is asserted there."""
    s = setups()[name]
    five = records(s.ys, s.spans)
    for flags in s.same_kernel_flags:
        wave_chooses_tier = bool(flags & THREAD) and name.startswith(('sgp', 'cd_sgp')) and name not in CUSTOM
        plain = s.run(five[1:2], flags=flags)
        for ys in (five[1:2], five):
            flagged = s.run(ys, flags=flags, missing='skip')
            at = 0 if ys.shape[0] == 1 else 1
            for g, w, what in zip(flagged, plain, ('mfs', 'Pfs', 'nll')):
                if wave_chooses_tier and ys.shape[0] > 1:
                    assert cs.max_rel_err(g[at], w[0]) <= GATE, (name, hex(flags), what, cs.max_rel_err(g[at], w[0]))
                else:
                    assert np.array_equal(g[at], w[0]), (name, hex(flags), what, ys.shape[0])


@pytest.mark.parametrize('name', ['ekf-chirp-e1', 'ekf-chirp-mix', 'sgp_gh3-chirp-e1', 'sgp_cub-chirp-mix', 'cd_ekf-chirp-e1', 'cd_sgp-chirp-e1',
                                  'ekf-lascala-e1', 'kf-linear3'])
def test_causality_and_restart(name):
    """Rows 0 .. 127 do not know what follows them; the filter restarted from row 191 (the end of a gap of a whole chunk) reproduces the rest:
    bit for bit on the generic kernels, within 1e-9 of the generic kernel's flagged launch on the matrix-core ones."""
    s = setups()[name]
    ys = records(s.ys, s.spans)[0:1]
    matrix_core = name.split('-')[0] in ('ekf', 'sgp_gh3', 'sgp_cub', 'cd_ekf', 'cd_sgp')
    for flags in (0, THREAD, GENERIC | WAVE):
        full = s.run(ys, flags=flags, missing='skip')
        head = s.run(ys[:, :128], flags=flags, missing='skip')
        for g, w, what in zip(head, full, ('mfs', 'Pfs', 'nll')):
            assert np.array_equal(g[0], w[0, :128]), (name, hex(flags), what)
        tail = s.run(ys[:, 192:], flags=flags, missing='skip', m0=full[0][0, 191], P0=full[1][0, 191])
        generic = not (matrix_core and flags == 0)
        if generic:
            assert np.array_equal(tail[0][0], full[0][0, 192:]) and np.array_equal(tail[1][0], full[1][0, 192:]), (name, hex(flags))
        else:
            ref = s.run(ys[:, 192:], flags=GENERIC | WAVE, missing='skip', m0=full[0][0, 191], P0=full[1][0, 191])
            errs = [cs.max_rel_err(tail[i][0], ref[i][0]) for i in range(3)]
            print(f'{name} restart on the matrix cores against the generic kernel: {errs}')
            assert max(errs) <= GATE, (name, errs)
        assert cs.max_rel_err(tail[2][0] + full[2][0, 191], full[2][0, 192:]) <= GATE


@pytest.mark.parametrize('name', ['ekf-chirp-e1', 'ekf-chirp-mix', 'ekf-lascala-e1'])
def test_ekf_kernel_for_gaps_against_the_generic_kernel(name):
    """The matrix-core EKF for records with gaps (cgp_mfma4.hpp: ekf4_gaps_kernel) against the flagged generic kernel, on the batch."""
    s = setups()[name]
    ys = batch_of(s, 5)
    got, ref = s.run(ys, missing='skip'), s.run(ys, flags=GENERIC | WAVE, missing='skip')
    errs = [cs.max_rel_err(g, w) for g, w in zip(got, ref)]
    print(f'{name}: the kernel for gaps against the generic kernel {errs}')
    assert max(errs) <= GATE, (name, errs)
    check_identities(s, ys, got[2], got[0], got[1])


def test_ekf_kernel_for_gaps_outside_the_wide_steps_domain():
    """A start state of 707 (as test_gpu_parity.py::test_sigma_point_filters_on_records_outside_the_lean_regime): beyond the wide step's
    |u2| < 700, so the chunk is repeated on the checked step -- counted by the kernel -- and still agrees with the generic kernel."""
    import bench
    from chirpgp_amd import models as pm, _engine
    fs = _fs()
    _, _, disc, m0, P0, H = pm.build_chirp_model(np.array([0.1, 0.1, 0.1, 1., 1., 707.]))
    ys = records(bench.chirp_batch(1, 262, 5, Xi=0.1, offset=8.0)[0], SPANS)
    _engine.debug_set(_engine.DBG_COUNT_REGIMES, 1)
    _engine.debug_counters(reset=True)
    got = fs.ekf(disc, H, 0.1, m0, P0, 1e-3, ys, missing='skip')
    rg = _engine.debug_counters(reset=True)
    _engine.debug_set(_engine.DBG_COUNT_REGIMES, 0)
    ref = fs.ekf(disc, H, 0.1, m0, P0, 1e-3, ys, flags=GENERIC | WAVE, missing='skip')
    errs = [cs.max_rel_err(g, w) for g, w in zip(got, ref)]                  # (asserts equal NaN positions too)
    print(f'start at 707: {rg} {errs}')
    assert rg['checked'] > 0 and rg['checked'] + rg['wide'] == 5 * 5, rg     # five records of five chunks
    assert max(errs) <= GATE, errs


def test_what_the_flag_must_not_change():
    from oracle import np_filters as onp
    s = setups()['sgp_gh3-chirp-e1']
    c = cs.chirp_case(T=262)
    fs = _fs()
    five = records(s.ys, s.spans)
    # a diverged filter (the first pivot of P0 fails) with finite measurements: NaN where it is NaN without the flag
    badP0 = np.array(c.P0)
    badP0[0, 0] = -1.0
    for flags in (0, GENERIC, THREAD):
        plain = fs.sgp_filter(c.disc, c.sgps, c.H, c.Xi, c.m0, badP0, c.dt, five[1:2], flags=flags)
        flagged = fs.sgp_filter(c.disc, c.sgps, c.H, c.Xi, c.m0, badP0, c.dt, five[1:2], flags=flags, missing='skip')
        assert np.isnan(plain[2]).all() and np.isnan(plain[0]).all()
        for g, w in zip(flagged, plain):
            assert np.array_equal(np.isnan(g), np.isnan(w)), hex(flags)
    # +inf is a measurement, not a gap
    ys = np.array(five[1:2])
    ys[0, 10] = np.inf
    for name in ('ekf-chirp-e1', 'sgp_gh3-chirp-e1', 'cd_ekf-chirp-e1', 'kf-linear3'):
        t = setups()[name]
        ysn = np.array(records(t.ys, t.spans)[1:2])
        ysn[0, 10] = np.inf
        for flags in (0, GENERIC, THREAD):
            plain, flagged = t.run(ysn, flags=flags), t.run(ysn, flags=flags, missing='skip')
            assert not np.isfinite(flagged[0][0, 10]).all() and not np.isfinite(flagged[2][0, 10])
            for g, w in zip(flagged, plain):
                assert np.array_equal(np.isfinite(g), np.isfinite(w)), (name, hex(flags))
    # without the flag a NaN measurement is the reference's poison, as before
    got = fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, five)
    for b in range(5):
        want = onp.ekf(c.o_disc, c.H, c.Xi, c.m0, c.P0, c.dt, five[b])
        for g, w in zip(got, want):
            assert cs.max_rel_err(g[b], w) <= GATE                        # (asserts equal NaN positions too)
    assert np.isnan(got[0][0]).all() and np.isfinite(got[0][1]).all()
    for bad in ('drop', True, 0):
        with pytest.raises(ValueError):
            fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, five, missing=bad)
    assert np.array_equal(fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, five, missing='propagate')[0], got[0], equal_nan=True)


@pytest.mark.parametrize('name', ['ekf-chirp-e1', 'sgp_gh3-chirp-e1', 'cd_ekf-chirp-e1', 'cd_sgp-chirp-e1'])
def test_smoothers_on_a_gapped_filter_result(name):
    """The smoothers need no flag: they read (mfs, Pfs) and predict again."""
    s = setups()[name]
    ys = records(s.ys, s.spans)[0]
    mfs, Pfs, _ = s.run(ys, missing='skip')
    got = s.smooth(mfs, Pfs)
    wm, wP, _ = (a[0] for a in oracle_rows(name))
    want = s.osmooth(wm, wP)
    errs = [cs.max_rel_err(g, w) for g, w in zip(got, want)]
    print(f'{name} smoother on gapped rows: {errs}')
    assert max(errs) <= GATE, (name, errs)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


def test_mle_on_a_gapped_record():
    from chirpgp_amd import mle, models as pm
    from oracle import np_filters as onp, np_models as om
    c = cs.chirp_case(T=262)
    ys = go.with_gaps(c.ys, SPANS)
    rng = np.random.default_rng(5)
    theta0 = pm.g_inv(np.array([0.1, 0.1, 0.1, 1., 1., 7.]))
    thetas = np.vstack([theta0, theta0 + 0.05 * rng.standard_normal((12, 6))])                       # 13 probes of one record
    got = mle.batched_nll('ekf', pm.build_chirp_model, thetas, ys, c.Xi, c.dt, missing='skip')
    want = []
    for th in thetas:
        _, _, o_disc, m0, P0, H = om.build_chirp_model(pm.g(th))
        want.append(go.gapped(onp.ekf, o_disc, H, c.Xi, m0, P0, c.dt, ys)[2][-1])
    assert cs.max_rel_err(got, np.array(want)) <= GATE, cs.max_rel_err(got, np.array(want))
    assert np.isnan(mle.batched_nll('ekf', pm.build_chirp_model, thetas, ys, c.Xi, c.dt)).all()       # (and poison without the keyword)
    f, g = mle.make_objective('ekf', pm.build_chirp_model, ys, c.Xi, c.dt, missing='skip')(theta0)
    assert abs(f - want[0]) <= GATE * abs(want[0]) and np.isfinite(g).all() and np.abs(g).max() > 0
    with pytest.raises(ValueError, match='tangent kernels know no gaps'):
        mle.fit('ekf', pm.build_chirp_model, [0.1, 0.1, 0.1, 1., 1., 7.], ys, c.Xi, c.dt, missing='skip', exact=True)
    with pytest.raises(ValueError, match='tangent kernels know no gaps'):
        mle.fit_many('ekf', pm.build_chirp_model, [0.1, 0.1, 0.1, 1., 1., 7.], ys[None, :], c.Xi, c.dt, missing='skip', exact=True)


def test_time_split_refuses_the_flag():
    from chirpgp_amd import _engine as E
    fs = _fs()
    c = cs.chirp_case(T=262)
    with pytest.raises(ValueError, match='time_split'):
        fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, c.ys, missing='skip', time_split=(2, 64))
    # the C-ABI itself: the flag handed over as a raw bit, with two segments and with one
    for segments in (2, 1):
        with pytest.raises(RuntimeError, match='CGP_SKIP_MISSING'):
            fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, c.ys, flags=E.SKIP_MISSING, time_split=(segments, 64))
    assert np.isfinite(fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, c.ys, time_split=(2, 64))[0]).all()         # (and still there without it)


def test_demo_runs(tmp_path):
    out = tmp_path / 'gappy.npz'
    subprocess.run([sys.executable, os.path.join(ROOT, 'demos', 'gappy_record.py'), '--T', '600', '--maxiter', '3', '--out', str(out)], check=True,
                   cwd=ROOT, timeout=300)
    res = np.load(out)
    for key in res.files:
        assert np.isfinite(res[key]).all(), key
    assert res['rmse_observed'] > 0 and res['rmse_gaps'] > 0
