"""Every kernel writes all of its outputs and nothing else, and reads nothing beyond its inputs: the guard-band sweep.

Each case runs an entry point of chirpgp_amd._engine twice on the same numbers -- once plainly, once with every large input copied into
a tests/guard_bands.py arena and every output handed out by that arena through _engine._new_output -- in two placements: payloads on
multiples of 256 bytes, and payloads 8 bytes off a 16-byte boundary.  After the guarded run

  1. no guard word has changed and no output word still holds the pre-fill (Arena.check),
  2. every output equals the plain run's bit for bit, NaNs included (the guards of the inputs hold NaN, so a read beyond an input that
     reaches the arithmetic shows here),
  3. the arena was asked for exactly the outputs the call wants,
  4. and after a refused call every output word still holds the pre-fill.

The shapes are the smallest at which a store window, a ragged tail or a tile edge exists; flags force the launch shape.  The cases that
go through route_filter / route_smoother are data (SWEEP, built at import, no GPU needed): each states the route it means to reach, and
tests/test_guard_bands_host.py asks the library's own route functions whether it does, and whether the sweep reaches every route there is.
The kernels of the lane routes (cgp_lane4.hpp) admit 16-byte aligned inputs only: their cases keep the inputs aligned in the 'odd'
placement too (`keep_aligned`), so that it is the OUTPUTS that sit 8 bytes off -- with misaligned inputs the launch takes the generic lane
kernel, which the generic_lane cases cover."""
import copy
import itertools
import math

import numpy as np
import pytest

from tests import guard_bands as gb
from tests import route_cases as rc

pytestmark = pytest.mark.gpu

WAVE, THREAD, SEQ, GENERIC, DPP = rc.WAVE, rc.THREAD, rc.SEQUENTIAL_SCAN, rc.GENERIC, rc.DPP
FOUR, TSPLIT, NOSPLIT, SKIP = rc.FOUR_TRIALS, rc.TIME_SPLIT, rc.NO_TIME_SPLIT, 0x2000
# the models of tests/route_cases.py and two more linear ones (the tile-layout smoother at its smallest and largest d)
MODELS = dict(rc.MODELS, linear5=(0, 5, 0, 'disc'), linear8=(0, 8, 0, 'disc'))

ALL7 = [w for w in itertools.product((True, False), repeat=3) if any(w)]
FULL = [(w, f) for w in ALL7 for f in ((False, True) if w[2] else (False,))]          # every want, nll_final_only on and off: 11
SHORT = [((True, True, True), False), ((True, True, True), True), ((True, False, False), False)]
LANE_SHAPES = [(1, 2), (63, 14), (64, 16), (65, 2), (70, 18), (129, 48)]             # where the 64-trial window has a short tail
SELECTIONS = [s for s in itertools.product((True, False), repeat=3) if any(s)]         # (mean, var, expect)

SWEEP = []


def routed(family, route, entry, method, model, B, T, flags, wave=1, sigma=None, segments=1, burn_in=0, null_rows=False, keep_aligned=False,
           split=None, **run):
    """One case that goes through the route functions.  `route`, `wave`: what it means to reach; `split`: whether the smoother's plan must
    have more than one segment (exact split: segs, with burn-in: bsegs).  `run`: what only the GPU run needs (variants, missing, records)."""
    cid = ('sel-' if entry == 'select' else '') + f'{route}-{method}-{model}-B{B}-T{T}-{flags:x}' + (f'-s{segments}' if segments > 1 else '') + ('-null' if null_rows else '') + run.pop('tag', '')
    assert cid not in {c['id'] for c in SWEEP}, cid
    SWEEP.append(dict(id=cid, family=family, route=route, wave=wave, entry=entry, method=method, model=model, sigma=sigma, B=B, T=T,
                      flags=flags | (SKIP if run.get('missing') == 'skip' else 0), segments=segments, burn_in=burn_in, null_rows=null_rows,
                      keep_aligned=keep_aligned, split=split, run=run))


def probe_query(c, placement):
    """The case as tests/route_cases.probe_line takes it (a dict of our own: route_cases.case() would append to the pinned list)."""
    align = 0 if placement == 'aligned' or c['keep_aligned'] else 8
    return dict(entry=c['entry'], method=c['method'], model=c['model'], sigma=c['sigma'], B=c['B'], T=c['T'], flags=c['flags'],
                segments=c['segments'], align=align, num_cus=256, null_rows=c['null_rows'], burn_in=c['burn_in'])


# ---- filters ------------------------------------------------------------------------------------------------------------------------
for _B in (1, 3):
    for _T in (1, 63, 64, 65, 130):
        routed('ekf4_mfma', 'ekf4_mfma', 'filter', 'ekf', 'chirp', _B, _T, WAVE, variants=FULL)
        routed('ekf4_mfma_gaps', 'ekf4_mfma', 'filter', 'ekf', 'chirp', _B, _T, WAVE, variants=FULL, missing='skip', tag='-gaps')
    # a NaN measurement without the flag poisons its trial from there on: NaNs compare bit for bit too
    routed('ekf4_mfma', 'ekf4_mfma', 'filter', 'ekf', 'chirp', _B, 65, WAVE, variants=SHORT, poison=True, tag='-nan')
    routed('ekf4_mfma_seg', 'ekf4_mfma_seg', 'filter_split', 'ekf', 'chirp', _B, 130, 0, segments=2, burn_in=64, variants=FULL)
for _B in (1, 4, 5, 7):
    for _T in (1, 65):
        routed('ekf4_mfma_x4', 'ekf4_mfma_x4', 'filter', 'ekf', 'chirp', _B, _T, FOUR | WAVE, variants=FULL)
for _route, _method, _model, _sigma, _flags in (
        ('ekf4_coop', 'ekf', 'chirp', None, DPP | WAVE), ('kf4_mfma', 'ekf', 'linear4', None, WAVE),
        ('sgp4_mfma', 'sgp', 'chirp', 'gh3', WAVE), ('sgp4_coop', 'sgp', 'chirp', 'gh3', DPP | WAVE),
        ('cdekf4_mfma', 'cd_ekf', 'chirp_sde1', None, WAVE), ('cdekf4_coop', 'cd_ekf', 'chirp_sde1', None, DPP | WAVE),
        ('cdsgp4_mfma', 'cd_sgp', 'chirp_sde1', 'gh3', WAVE), ('cdsgp4_coop', 'cd_sgp', 'chirp_sde1', 'gh3', DPP | WAVE)):
    for _T in (1, 64, 65):
        routed(_route, _route, 'filter', _method, _model, 3, _T, _flags, sigma=_sigma, variants=FULL)
for _route, _method, _sigma in (('lane4_ekf', 'ekf', None), ('lane4_sgp', 'sgp', 'gh3')):
    for _B, _T in LANE_SHAPES:
        routed(_route, _route, 'filter', _method, 'chirp', _B, _T, THREAD, wave=0, sigma=_sigma, keep_aligned=True, variants=FULL)
    # shared records: 5 records of which an index picks and orders, 13 trials each; one record for 70 trials
    routed(_route, _route, 'filter', _method, 'chirp', 65, 14, THREAD, wave=0, sigma=_sigma, keep_aligned=True, variants=SHORT,
           records=5, tpr=13, ridx=(4, 0, 3, 1, 2), tag='-indexed')
    routed(_route, _route, 'filter', _method, 'chirp', 70, 18, THREAD, wave=0, sigma=_sigma, keep_aligned=True, variants=SHORT, records=1, tpr=70,
           tag='-shared')
    routed(_route, _route, 'filter', _method, 'chirp', 70, 18, THREAD, wave=0, sigma=_sigma, keep_aligned=True, variants=SHORT, poison=True, tag='-nan')
# the generic kernels: one lane per trial at an odd T (the lane kernels take even T only), one wavefront per trial on what has no kernel of its own
routed('generic', 'generic_lane', 'filter', 'ekf', 'chirp', 65, 15, THREAD, wave=0, variants=FULL)
routed('generic', 'generic_lane', 'filter', 'sgp', 'chirp', 65, 15, THREAD, wave=0, sigma='gh3', variants=SHORT)
routed('generic', 'generic_lane', 'filter', 'ekf', 'harm2', 65, 15, THREAD, wave=0, variants=SHORT)
routed('generic', 'generic_lane', 'filter', 'ekf', 'chirp', 65, 16, THREAD | GENERIC, wave=0, variants=SHORT, missing='skip', tag='-gaps')
for _T in (1, 65):
    routed('generic', 'generic_wave', 'filter', 'ekf', 'linear3', 3, _T, WAVE, variants=SHORT)
    routed('generic', 'generic_wave', 'filter', 'sgp', 'linear3', 3, _T, WAVE, sigma='gh3', variants=SHORT)
    routed('generic', 'generic_wave', 'filter', 'ekf', 'harm4', 3, _T, WAVE, variants=SHORT)
    routed('generic', 'generic_wave', 'filter', 'cd_ekf', 'linear_sde4', 3, _T, WAVE, variants=SHORT)
    routed('generic', 'generic_wave', 'filter', 'cd_sgp', 'linear_sde4', 3, _T, WAVE, sigma='gh3', variants=SHORT)
for _T in (1, 33, 64, 65):
    for _model in ('harm2', 'harm3'):
        routed('coop8_filters', 'ekf8_coop', 'filter', 'ekf', _model, 2, _T, WAVE, variants=SHORT)
        routed('coop8_filters', 'sgp8_coop', 'filter', 'sgp', _model, 2, _T, WAVE, sigma='cub', variants=SHORT)
for _T in (1, 65):
    for _model in ('kpt1', 'kpt2', 'kpt3'):
        routed('kpt', 'kpt8_coop', 'filter', 'ekf_kpt', _model, 2, _T, WAVE, variants=SHORT)
    routed('kpt', 'generic_kpt', 'filter', 'ekf_kpt', 'kpt2', 2, _T, WAVE | GENERIC, variants=SHORT)
    routed('kpt', 'generic_kpt', 'filter', 'ekf_kpt', 'kpt3', 65, _T, THREAD, wave=0, variants=SHORT)

# ---- smoothers ----------------------------------------------------------------------------------------------------------------------
SMOOTHER_T = (1, 2, 64, 65, 66, 130)
for _B in (1, 3):
    for _route, _method, _model, _sigma in (('walk4_linear', 'eks', 'linear4', None), ('walk4_harm', 'eks', 'chirp', None),
                                            ('walk4_harm', 'sgp', 'chirp', 'gh3'), ('coop8_linear', 'eks', 'linear5', None),
                                            ('coop8_linear', 'eks', 'linear8', None), ('coop8_harm', 'eks', 'harm2', None),
                                            ('coop8_harm', 'sgp', 'harm3', 'cub')):
        _family = 'walk4' if _route.startswith('walk4') else 'coop8_smoothers'
        for _T in SMOOTHER_T:
            routed(_family, _route, 'smoother', _method, _model, _B, _T, WAVE | NOSPLIT, sigma=_sigma, split=False)
        for _T in (130, 200):                                 # the exact split: 3 and 4 tiles, one a segment
            routed(_family, _route, 'smoother', _method, _model, _B, _T, WAVE | TSPLIT, sigma=_sigma, split=True)
    for _T in SMOOTHER_T:
        # the generic smoothers: the time-parallel scan, step by step, one lane per trial
        for _route, _model in (('disc_linear', 'linear3'), ('disc_harm', 'chirp')):
            routed('disc', _route, 'smoother', 'eks', _model, _B, _T, WAVE | GENERIC)
            routed('disc', _route, 'smoother', 'eks', _model, _B, _T, WAVE | SEQ)
            routed('disc', _route, 'smoother', 'eks', _model, _B, _T, THREAD | GENERIC, wave=0)
        routed('disc', 'disc_harm', 'smoother', 'sgp', 'chirp', _B, _T, WAVE | GENERIC, sigma='gh3')
        for _route, _method, _model, _sigma, _flags in (
                ('sde_linear', 'cd_eks', 'linear_sde4', None, WAVE), ('sde_linear', 'cd_sgp', 'linear_sde4', 'gh3', WAVE),
                ('sde_harm', 'cd_eks', 'chirp_sde2', None, WAVE), ('sde_harm', 'cd_eks', 'chirp_sde1', None, WAVE | GENERIC),
                ('cdeks4_mfma', 'cd_eks', 'chirp_sde1', None, WAVE), ('cdeks4_coop', 'cd_eks', 'chirp_sde1', None, WAVE | DPP),
                ('cdsgps4_mfma', 'cd_sgp', 'chirp_sde1', 'gh3', WAVE), ('cdsgps4_coop', 'cd_sgp', 'chirp_sde1', 'gh3', WAVE | DPP)):
            routed('sde', _route, 'smoother', _method, _model, _B, _T, _flags, sigma=_sigma)
    for _route, _method, _sigma in (('cdeks4_mfma', 'cd_eks', None), ('cdsgps4_mfma', 'cd_sgp', 'gh3')):
        # the split with burn-in: two segments of one chunk each; a record of one chunk, which is not split
        routed('sde', _route, 'smoother_split', _method, 'chirp_sde1', _B, 130, WAVE, sigma=_sigma, segments=2, burn_in=64, split=True)
        routed('sde', _route, 'smoother_split', _method, 'chirp_sde1', _B, 65, WAVE, sigma=_sigma, segments=5, burn_in=64, split=False)
for _method, _model in (('eks', 'chirp'), ('cd_eks', 'chirp_sde1')):
    for _B, _T in LANE_SHAPES + [(65, 3), (70, 15), (129, 49)]:
        routed('lane4_smoothers', 'lane4', 'smoother', _method, _model, _B, _T, THREAD, wave=0, keep_aligned=True)

# ---- selected outputs: a walk, the tile layout, the lane kernel, and a route that gathers them from its full rows
for _T in (2, 65):
    for _route, _model, _B, _flags, _wave, _keep in (('walk4_harm', 'chirp', 3, WAVE | NOSPLIT, 1, False), ('coop8_harm', 'harm2', 3, WAVE | NOSPLIT, 1, False),
                                                     ('lane4', 'chirp', 65, THREAD, 0, True), ('disc_linear', 'linear3', 3, WAVE, 1, False)):
        for _rows in (True, False):
            if _route == 'disc_linear' and not _rows:
                # refused by the library (NULL rows on a gather route); _engine.run_smoother then hands it temporary rows: the same
                # launch as with rows, stated as that
                routed('select', _route, 'select', 'eks', _model, _B, _T, _flags, wave=_wave, keep_aligned=_keep, rows=False, tag='-norows')
            else:
                routed('select', _route, 'select', 'eks', _model, _B, _T, _flags, wave=_wave, null_rows=not _rows, keep_aligned=_keep, rows=_rows)


# ---- the models, their data ----------------------------------------------------------------------------------------------------------
class Data:
    pass


def model_data(name, B, per_trial, seed=0):
    """Descriptor, operands (NumPy) and dt of a model of MODELS; per_trial: parameters, H, Xi, m0, P0 carry the batch axis."""
    from chirpgp_amd import _engine as E, models as pm
    model_id, d, nh, kind = MODELS[name]
    rng = np.random.default_rng(1000 + seed)
    lead = (B,) if per_trial else ()
    jitter = lambda n: 1 + 0.2 * rng.random(lead + (n,))
    m = Data()
    m.d, m.kind, m.gamma, m.dt = d, kind, None, 1e-3
    m.H = None
    if name.startswith('linear'):
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        m.H, m.m0, m.P0 = np.r_[1., 0.5 * rng.standard_normal(d - 1)], 0.1 * rng.standard_normal(d), np.eye(d)
        if kind == 'disc':
            F = 0.8 * q * jitter(1)[..., None]                # (a contraction whatever the jitter: 0.8 .. 0.96 times a rotation)
            m.spec, m.dt = pm.linear_cond_m_cov(F, 0.01 * (np.eye(d) + 0.1 * q @ q.T)), 0.
        else:
            A = (-np.eye(d) + 3. * (q - q.T)) * jitter(1)[..., None]
            m.spec, disp = pm.linear_sde(A, 0.3 * np.eye(d))
            m.gamma = disp.outer()
        if per_trial:
            m.H, m.m0, m.P0 = np.tile(m.H, (B, 1)) * jitter(d), np.tile(m.m0, (B, 1)) * jitter(d), np.eye(d) * jitter(1)[..., None]
    elif kind == 'kpt':
        F, Sigma, m.m0, m.P0, _ = pm.build_kpt_chirp_model(np.array([0.5, 1e-4, 0.1, 8., 1.]) * jitter(5), 1000., nh)
        m.spec = pm.linear_cond_m_cov(F, Sigma)
        m.spec.model_id, m.spec.n_harm = pm.M_KPT, nh
    else:
        if model_id == 2:
            drift, disp, disc, m.m0, m.P0, m.H = pm.build_lascala_model(np.array([0.1, 1., 1., 7.]) * jitter(4))
        else:
            drift, disp, disc, m.m0, m.P0, m.H = pm.build_harmonic_chirp_model(np.array([0.1, 0.1, 0.1, 1., 1., 7.]) * jitter(6), nh)
        m.spec = disc if kind == 'disc' else drift
        if kind == 'sde':
            m.gamma = disp.outer()
        if per_trial:
            m.H = np.tile(m.H, (B, 1)) * jitter(d)
    m.Xi = 0.1 * jitter(1)[..., 0] if per_trial else 0.1
    m.filter = {'disc': E.F_EKF, 'sde': E.F_CD_EKF, 'kpt': E.F_EKF_KPT}[kind]
    return m


def sigma_points(kind, d):
    from chirpgp_amd.quadratures import SigmaPoints
    return None if kind is None else SigmaPoints.gauss_hermite(d, 3) if kind == 'gh3' else SigmaPoints.cubature(d)


def records(R, T, seed=0):
    rng = np.random.default_rng(2000 + seed)
    return np.sin(2 * math.pi * 7e-3 * np.arange(T) + rng.random((R, 1))) + 0.1 * rng.standard_normal((R, T))


class Inputs:
    """The large inputs of a call, as plain device tensors or taken from an arena (per input: `aligned` overrides the arena's placement)."""

    def __init__(self, arena=None, keep_aligned=False):
        self.arena, self.placement = arena, ('aligned' if keep_aligned else None)

    def __call__(self, x, name):
        import torch
        if x is None:
            return None
        if self.arena is not None:
            from chirpgp_amd import _engine as E
            view = self.arena.input(x, name, self.placement)
            assert E.dev(view).data_ptr() == view.data_ptr() == E.dev_const(view).data_ptr()       # what the kernel is handed IS the guarded array
            return view
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
        return t.to('cuda').contiguous()

    def model(self, m):
        """-> (spec with its parameters in place, H, Xi, m0, P0) of a model_data."""
        spec = copy.copy(m.spec)
        spec.params = self(m.spec.params, 'params')
        return spec, self(m.H, 'H'), self(np.atleast_1d(m.Xi), 'Xi'), self(m.m0, 'm0'), self(m.P0, 'P0')


def flat(res):
    """The tensors of a result, in order: tuples and the selection dict opened up, None kept."""
    out = []
    for r in res if isinstance(res, (tuple, list)) else (res,):
        if isinstance(r, dict):
            out += [r.get(k) for k in ('mean', 'var', 'expect')]
        else:
            out.append(r)
    return out


LAUNCHES = [0]                     # guarded launches so far (reported by the last test of the file)


def guarded(call, placement, keep_aligned, expect, what, plain=None, finite=True):
    """`call(inputs)` plainly and inside an arena of `placement`; the four assertions of the module's docstring but the refusals.
    `expect`: the names the seam must be asked for, in any order."""
    import torch
    if plain is None:
        plain = flat(call(Inputs()))
    # (the cases are sound ones: a sweep whose results are NaN throughout would compare nothing)
    assert not finite or all(p is None or bool(torch.isfinite(p).all()) for p in plain), (what, 'the plain run is not finite')
    arena = gb.Arena('cuda', placement)
    with arena.installed():
        got = flat(call(Inputs(arena, keep_aligned)))
    LAUNCHES[0] += 1
    assert arena.check() == [], (what, placement)
    assert sorted(n for n, _ in arena.requests) == sorted(expect), (what, arena.requests, expect)
    assert len(got) == len(plain), what
    for k, (g, p) in enumerate(zip(got, plain)):
        assert gb.same_bits(g, p), (what, placement, f'output {k} differs from the plain run',
                                    None if g is None or p is None else float((g - p).abs().nan_to_num(nan=math.inf).max()))
    want_ptr = (lambda p: p % 16 == 8) if placement == 'odd' else (lambda p: p % 256 == 0)
    assert all(want_ptr(b.payload.data_ptr()) for b in arena.blocks if b.kind == 'output'), what
    assert all(isinstance(g, torch.Tensor) or g is None for g in got)
    return plain


def refused(call, placement, what):
    """A call the library refuses: RuntimeError with its message, every output word still pre-filled, every guard intact."""
    arena = gb.Arena('cuda', placement)
    with arena.installed():
        with pytest.raises(RuntimeError, match=r'failed \(-\d+\)'):
            call(Inputs(arena))
    import torch
    torch.cuda.synchronize()
    assert arena.requests, what                       # (the refusal came from the library, behind the allocations)
    assert arena.guard_violations() == [] and arena.written() == [], (what, placement)


def cases_of(family):
    return [c for c in SWEEP if c['family'] == family]


FILTER_FAMILIES = sorted({c['family'] for c in SWEEP if c['entry'].startswith('filter')})
SMOOTHER_FAMILIES = sorted({c['family'] for c in SWEEP if c['entry'].startswith('smoother')})


# ---- the routed sweep ----------------------------------------------------------------------------------------------------------------
def run_filter_case(c, placement):
    from chirpgp_amd import _engine as E
    run, B, T = c['run'], c['B'], c['T']
    R = run.get('records', B)
    m = model_data(c['model'], B, per_trial=B > 1 and 'records' not in run, seed=T)
    sg = sigma_points(c['sigma'], m.d)
    ys = records(R, T, seed=B)
    if run.get('missing'):
        ys[:, -1] = np.nan                                                    # a gap in the last step
        if T > 3:
            ys[0, 1] = np.nan
    if run.get('poison'):
        ys[R // 2, T // 2] = np.nan
    kw = dict(flags=c['flags'] & ~SKIP, missing=run.get('missing'), trials_per_record=run.get('tpr'),
              record_index=None if run.get('ridx') is None else np.array(run['ridx']))
    if c['entry'] == 'filter_split':
        kw.update(time_split=(c['segments'], c['burn_in']), return_junction_error=True)
    method = {'ekf': E.F_EKF, 'sgp': E.F_SGP, 'cd_ekf': E.F_CD_EKF, 'cd_sgp': E.F_CD_SGP, 'ekf_kpt': E.F_EKF_KPT}[c['method']]
    for want, final in run['variants']:
        def call(inp):
            spec, H, Xi, m0, P0 = inp.model(m)
            return E.run_filter(method, spec, sg, m.gamma, H, Xi, m0, P0, m.dt, inp(ys, 'ys'), nll_final_only=final, want=want, **kw)
        expect = [n for n, on in zip(('mfs', 'Pfs', 'nll'), want) if on] + (['junction_err'] if c['entry'] == 'filter_split' else [])
        guarded(call, placement, c['keep_aligned'], expect, (c['id'], want, final), finite=not run.get('poison'))


_filtered = {}


def filtering_rows(model, B, T):
    """mfs, Pfs (device tensors) for a smoother case: the model's EKF (cd_ekf for an SDE) by its default launch, once per shape."""
    from chirpgp_amd import _engine as E
    key = (model, B, T)
    if key not in _filtered:
        if len(_filtered) > 64:
            _filtered.clear()
        m = model_data(model, B, per_trial=B > 1, seed=T)
        f = E.run_filter(m.filter, m.spec, None, m.gamma, m.H, m.Xi, m.m0, m.P0, m.dt, E.dev(records(B, T, seed=B)), want=(True, True, False))
        _filtered[key] = (m, f[0], f[1])
    return _filtered[key]


def run_smoother_case(c, placement):
    from chirpgp_amd import _engine as E
    m, mfs, Pfs = filtering_rows(c['model'], c['B'], c['T'])
    sg = sigma_points(c['sigma'], m.d)
    method = {'eks': E.S_EKS, 'sgp': E.S_SGP, 'cd_eks': E.S_CD_EKS, 'cd_sgp': E.S_CD_SGP}[c['method']]
    variants = [None]
    if c['entry'] == 'select':
        variants = SELECTIONS
    for sel in variants:
        kw, expect = dict(flags=c['flags']), ['mss', 'Pss']
        if c['entry'] == 'smoother_split':
            kw.update(time_split=(c['segments'], c['burn_in']), return_junction_error=True)
            expect.append('junction_err')
        if sel is not None:
            rows = c['run']['rows']
            kw.update(select=dict(comp=-2, mean=sel[0], var=sel[1], expect='softplus' if sel[2] else None, order=10), want=(rows, rows))
            expect = [n for n, on in zip(('comp_mean', 'comp_var', 'expect'), sel) if on]
            expect += ['mss', 'Pss'] if rows else [] if c['null_rows'] else ['mss (temporary)', 'Pss (temporary)']

        def call(inp):
            spec = copy.copy(m.spec)
            spec.params = inp(m.spec.params, 'params')
            return E.run_smoother(method, spec, sg, m.gamma, m.dt, inp(mfs, 'mfs'), inp(Pfs, 'Pfs'), **kw)
        guarded(call, placement, c['keep_aligned'], expect, (c['id'], sel))


@pytest.mark.parametrize('placement', gb.PLACEMENTS)
@pytest.mark.parametrize('family', FILTER_FAMILIES)
def test_filters(family, placement):
    for c in cases_of(family):
        run_filter_case(c, placement)


@pytest.mark.parametrize('placement', gb.PLACEMENTS)
@pytest.mark.parametrize('family', SMOOTHER_FAMILIES)
def test_smoothers(family, placement):
    for c in cases_of(family):
        run_smoother_case(c, placement)


@pytest.mark.parametrize('placement', gb.PLACEMENTS)
def test_selected_outputs(placement):
    for c in cases_of('select'):
        run_smoother_case(c, placement)


# ---- models compiled at run time -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('placement', gb.PLACEMENTS)
def test_custom_models(placement):
    """run_filter_custom and run_smoother_custom on the Lorenz-63 source of tests/test_gpu_custom.py: the generic lane kernel on it."""
    from chirpgp_amd import _engine as E, models as pm
    from tests.test_gpu_custom import LORENZ, KAPPA, LAM, MU
    B, T = 65, 33
    p = np.array([KAPPA, LAM, MU, 25.]) * (1 + 0.01 * np.random.default_rng(3).random((B, 4)))
    disc = pm.custom_cond_m_cov(LORENZ, 3, p)
    H, m0, P0 = np.array([1., 0., 0.]), np.zeros(3), np.eye(3)
    ys = 5 * records(B, T)
    rows = {}
    for want, final in SHORT:
        def call(inp):
            spec = copy.copy(disc)
            spec.params = inp(p, 'params')
            return E.run_filter_custom(spec, None, inp(H, 'H'), inp(np.full(B, 2.), 'Xi'), inp(m0, 'm0'), inp(P0, 'P0'), 1e-3, inp(ys, 'ys'),
                                       nll_final_only=final, want=want)
        res = guarded(call, placement, False, [n for n, on in zip(('mfs', 'Pfs', 'nll'), want) if on], ('filter_custom', want, final))
        rows.setdefault('f', res)

    def smooth(inp):
        spec = copy.copy(disc)
        spec.params = inp(p, 'params')
        return E.run_smoother_custom(spec, None, 1e-3, inp(rows['f'][0], 'mfs'), inp(rows['f'][1], 'Pfs'))
    guarded(smooth, placement, False, ['mss', 'Pss'], 'smoother_custom')


# ---- sample paths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('placement', gb.PLACEMENTS)
@pytest.mark.parametrize('T', [1, 65])
def test_samples(T, placement):
    from chirpgp_amd import _engine as E
    B = 2
    for model, method, sigma in (('chirp', 'eks', None), ('chirp', 'sgp', 'cub'), ('linear4', 'eks', None)):
        m, mfs, Pfs = filtering_rows(model, B, T)
        sg = sigma_points(sigma, 4)
        for S in (1, 64, 65):
            if model != 'chirp' or sigma is not None:
                if S != 65:
                    continue
            z = np.random.default_rng(S).standard_normal((B, S, T, 4))
            for want_paths, select in ((True, None), (False, dict(comp=2, func='softplus')), (True, dict(comp=2, func='softplus'))):
                for normals in (None, z):
                    def call(inp):
                        spec = copy.copy(m.spec)
                        spec.params = inp(m.spec.params, 'params')
                        return E.run_smoother_sample(E.S_EKS if method == 'eks' else E.S_SGP, spec, sg, m.dt, inp(mfs, 'mfs'), inp(Pfs, 'Pfs'), S, seed=5,
                                                     normals=inp(normals, 'normals'), want_paths=want_paths, select=select)
                    expect = (['paths'] if want_paths else []) + (['comp_paths'] if select else [])
                    guarded(call, placement, False, expect, ('sample', model, method, S, T, want_paths, select, normals is not None))


# ---- gradient and Fisher entry points ---------------------------------------------------------------------------------------------------
ENTRIES = ('ekf_nll_grad', 'sgp_nll_grad', 'ekf_nll_fisher', 'sgp_nll_fisher', 'cd_ekf_nll_grad')


def tangent_call(entry, m, sg, ys, dirs):
    from chirpgp_amd import _engine as E

    def call(inp):
        spec, H, Xi, m0, P0 = inp.model(m)
        args = (H, Xi, m0, P0, m.dt, inp(ys, 'ys'), inp(dirs, 'dirs'))
        if entry == 'cd_ekf_nll_grad':
            return E.run_cd_ekf_nll_grad(spec, m.gamma, *args)
        if entry.startswith('sgp'):
            return getattr(E, 'run_' + entry)(spec, sg, *args)
        return getattr(E, 'run_' + entry)(spec, *args)
    return call


@pytest.mark.parametrize('placement', gb.PLACEMENTS)
@pytest.mark.parametrize('entry', ENTRIES)
def test_gradient_and_fisher_entries(entry, placement):
    """n_dir in {1, 6, 16} against B in {1, 5}: 64 / n_dir trials share a wavefront, and that number never divides B."""
    sg = sigma_points('cub', 4)
    for B in (1, 5):
        for T in (1, 65):
            m = model_data('chirp_sde1' if entry.startswith('cd') else 'chirp', B, per_trial=B > 1, seed=T)
            ys = records(B, T, seed=B)
            for n_dir in (1, 6, 16):
                dirs = 0.1 * np.random.default_rng(n_dir).standard_normal((B, n_dir, 27 if entry.startswith('cd') else 24))
                expect = ['nll', 'grad'] + (['fisher'] if entry.endswith('fisher') else [])
                guarded(tangent_call(entry, m, sg, ys, dirs), placement, False, expect, (entry, B, T, n_dir))


# ---- the input side ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('placement', gb.PLACEMENTS)
def test_simulate_add_noise_and_expectations(placement):
    from chirpgp_amd import _engine as E
    for model in ('chirp', 'linear3'):
        for B in (1, 65):
            m = model_data(model, B, per_trial=B > 1)
            for T in (1, 77, 78):                             # (an even T on an aligned array takes the two-word stores)
                for flags in (WAVE, THREAD):
                    for want in ((True, False), (False, True), (True, True)):
                        def call(inp):
                            spec, H, Xi, m0, P0 = inp.model(m)
                            return E.run_simulate(spec, H, Xi, m0, P0, m.dt, T, 11, B, want=want, flags=flags)
                        guarded(call, placement, False, [n for n, on in zip(('xs', 'ys'), want) if on], ('simulate', model, B, T, flags, want))
    for B, T, shared in ((1, 1, True), (3, 77, True), (65, 78, False), (3, 1, False)):
        clean = records(1, T)[0] if shared else records(B, T)
        guarded(lambda inp: E.add_noise(inp(clean, 'clean'), inp(np.full(B, 0.1), 'Xi'), 7, B), placement, False, ['ys'], ('add_noise', B, T, shared))
    xi, w = E._gh_rule(10)
    for n in (1, 65, 1000):
        rng = np.random.default_rng(n)
        ms, sd = rng.standard_normal(n), 0.1 + rng.random(n)
        guarded(lambda inp: E.gaussian_expectation(inp(ms, 'ms'), inp(sd, 'chol_Ps'), inp(xi, 'xi'), inp(w, 'w')), placement, False, ['out'],
                ('gaussian_expectation', n))


@pytest.mark.parametrize('placement', gb.PLACEMENTS)
def test_squared_error_sums_accumulate_inside_their_array(placement):
    """cgp_squared_error_sums adds into `sums`: guard checks only, the values against NumPy as tests/test_gpu_sim.py has them."""
    import torch
    from chirpgp_amd import _engine as E
    rng = np.random.default_rng(4)
    for B, T, d, comps in ((1, 1, 4, [2]), (65, 77, 4, [2, 0]), (513, 3, 6, [5, 0, 3])):
        a, r = rng.standard_normal((B, T, d)), rng.standard_normal((B, T, d))
        arena = gb.Arena('cuda', placement)
        sums = arena.output((len(comps), 2, T), 'sums')
        sums.zero_()
        for _ in range(2):                                   # twice: it accumulates
            out = E.squared_error_sums(arena.input(a, 'a'), arena.input(r, 'r'), comps, sums=sums)
        assert out.data_ptr() == sums.data_ptr()
        assert arena.check() == []
        e2 = (a - r)[:, :, comps] ** 2
        want = 2 * np.stack([e2.sum(0).T, (e2 ** 2).sum(0).T], axis=1)
        np.testing.assert_allclose(sums.cpu().numpy(), want, rtol=1e-12)
    assert isinstance(sums, torch.Tensor)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('placement', gb.PLACEMENTS)
def test_refused_calls_write_nothing(placement):
    from chirpgp_amd import _engine as E
    B, T = 3, 130
    m = model_data('chirp', B, True)
    s = model_data('chirp_sde1', B, True)
    h2 = model_data('harm2', B, True)
    ys = records(B, T)
    _, mfs, Pfs = filtering_rows('chirp', B, T)
    _, mfs6, Pfs6 = filtering_rows('harm2', B, T)

    def filt(method, mod, **kw):
        def call(inp):
            spec, H, Xi, m0, P0 = inp.model(mod)
            return E.run_filter(method, spec, None, mod.gamma, H, Xi, m0, P0, mod.dt, inp(ys, 'ys'), **kw)
        return call
    refused(filt(E.F_CD_EKF, m), placement, 'cd_ekf on a discrete model')
    refused(filt(E.F_EKF, m, time_split=(2, 64), flags=THREAD), placement, 'time-split filter, one lane per trial')
    refused(filt(E.F_EKF, h2, time_split=(2, 64)), placement, 'time-split ekf on two harmonics')
    refused(filt(E.F_EKF, m, time_split=(2, -1)), placement, 'negative burn-in')

    def smooth(method, mod, rows, **kw):
        def call(inp):
            return E.run_smoother(method, mod.spec, None, mod.gamma, mod.dt, inp(rows[0], 'mfs'), inp(rows[1], 'Pfs'), **kw)
        return call
    refused(smooth(E.S_CD_EKS, m, (mfs, Pfs)), placement, 'cd_eks on a discrete model')
    refused(smooth(E.S_EKS, m, (mfs, Pfs), time_split=(2, 64)), placement, 'burn-in split of a discrete smoother')
    refused(smooth(E.S_CD_EKS, s, (mfs, Pfs), time_split=(2, -1)), placement, 'negative burn-in')
    refused(smooth(E.S_EKS, m, (mfs, Pfs), select=dict(comp=2, expect='softplus', order=33)), placement, 'select: order 33')

    def sample(method, mod, rows, **kw):
        def call(inp):
            return E.run_smoother_sample(method, mod.spec, None, mod.dt, inp(rows[0], 'mfs'), inp(rows[1], 'Pfs'), 4, **kw)
        return call
    refused(sample(E.S_EKS, m, (mfs, Pfs), flags=WAVE), placement, 'sample: a flag')
    refused(sample(E.S_EKS, h2, (mfs6, Pfs6)), placement, 'sample: d = 6')
    refused(sample(E.S_EKS, m, (mfs, Pfs), trial0=-1), placement, 'sample: negative trial0')

    sg = sigma_points('cub', 4)
    for entry in ENTRIES:
        mod = s if entry.startswith('cd') else m
        per = 27 if entry.startswith('cd') else 24
        if entry.endswith('fisher'):
            refused(tangent_call(entry, mod, sg, ys, np.zeros((B, 17, per))), placement, f'{entry}: 17 directions')
        wrong = model_data('chirp_sde2' if entry.startswith('cd') else 'harm2', B, True)
        refused(tangent_call(entry, wrong, sigma_points('cub', 6), ys, np.zeros((B, 2, per))), placement, f'{entry}: d = 6')
        if not entry.startswith('cd'):
            refused(tangent_call(entry, s, sg, ys, np.zeros((B, 2, per))), placement, f'{entry}: an SDE model')

    def simulate(mod, **kw):
        def call(inp):
            spec, H, Xi, m0, P0 = inp.model(mod)
            return E.run_simulate(spec, H, Xi, m0, P0, mod.dt, T, 1, B, **kw)
        return call
    refused(simulate(s), placement, 'simulate: an SDE model')
    refused(simulate(m, trial0=-1), placement, 'simulate: negative trial0')
    refused(lambda inp: E.add_noise(inp(ys, 'clean'), 0.1, 1, B, trial0=-1), placement, 'add_noise: negative trial0')
    xi, w = E._gh_rule(10)
    refused(lambda inp: E.gaussian_expectation(inp(ys[0], 'ms'), inp(np.ones(T), 'chol_Ps'), xi, w, func=7), placement, 'expectation: unknown integrand')


@pytest.fixture(scope='module', autouse=True)
def launch_count():
    """Says (with `pytest -s`) how many guarded launches the file made; as many plain ones ran beside them."""
    yield
    print(f'\nguard-band sweep: {LAUNCHES[0]} guarded launches, {len(SWEEP)} routed cases')
