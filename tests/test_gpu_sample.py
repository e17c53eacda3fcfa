"""cgp_smoother_sample on the GPU: posterior sample paths of rts / eks / sgp_smoother against the NumPy restatement
(tests/sample_oracle.py), the Philox addressing, the joint law, the zero-column rule, records with gaps, NaN rows and the argument checks.

Gates.  Against the oracle: 10 x the distance of the NumPy walk from its 50-digit form (tests/test_sample_oracle.py (a)), per
(method, model), in units of the output's largest entry -- sample_oracle.GPU_GATE; with the Philox stream, plus the device Box-Muller's
1e-11.  Statistics: every entry of the sample mean, covariance and lag-one cross-covariance within 6 standard errors
(sample_oracle.moment_excess); the seed is fixed and the oracle passes with it (tests/test_sample_oracle.py (b)).

Measured on an MI355X (worst over the lengths and S = 5, 70; gates 1e-12, 1e-7, 1e-2, 2e-5, 2e-5): rts 3.5e-14, eks chirp 9.7e-9,
eks La Scala 1.2e-3, sgp chirp 2.1e-6, sgp La Scala 2.8e-6; joint law 2.4 - 3.0 standard errors (chirp), 1.4 - 3.3 (La Scala, M32 block)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sample_oracle as so

pytestmark = pytest.mark.gpu

TS = (1, 2, 63, 64, 65, 130)
B = 3
STAT_GATE, STAT_SEED = 6.0, 2024


def _fs():
    from chirpgp_amd import filters_smoothers as fs
    return fs


def _filter(p, ys, **kw):
    fs, c = _fs(), p.case
    if p.method == 'rts':
        return fs.kf(p.cond[0], p.cond[1], c.H, c.Xi, c.m0, c.P0, ys, **kw)[:2]
    if p.method == 'eks':
        return fs.ekf(c.disc, c.H, c.Xi, c.m0, c.P0, c.dt, ys, **kw)[:2]
    return fs.sgp_filter(c.disc, c.sgps, c.H, c.Xi, c.m0, c.P0, c.dt, ys, **kw)[:2]


@functools.lru_cache(maxsize=None)
def setup(name, T, nb=B):
    """Filtering rows of `nb` records from the engine's own filter, and the oracle's maps on those rows (computed once, never changed)."""
    p = so.pairs()[name]
    ys = np.stack([p.case.ys[:T] + 0.05 * b for b in range(nb)])
    mfs, Pfs = _filter(p, ys)
    maps = [so.oracle_maps(p, mfs[b], Pfs[b]) for b in range(nb)]
    return p, mfs, Pfs, maps


def rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def oracle_paths(mfs, Pfs, maps, z):
    return np.stack([so.walk(maps[b], mfs[b], Pfs[b], z[b])[0] for b in range(len(maps))])


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('name', list(so.GPU_GATE))
def test_given_normals_against_the_oracle(name, T):
    p, mfs, Pfs, maps = setup(name, T)
    gate = so.GPU_GATE[name]
    for S in (5, 70):
        z = np.random.default_rng(100 * T + S).standard_normal((B, S, T, 4))
        want = oracle_paths(mfs, Pfs, maps, z)
        both, soft = p.engine(_fs(), mfs, Pfs, S, normals=z, select=dict(comp=2, func='softplus'))
        alone, none = p.engine(_fs(), mfs, Pfs, S, normals=z)
        nopaths, ident = p.engine(_fs(), mfs, Pfs, S, normals=z, want_paths=False, select=dict(comp=1, func='identity'))
        nopaths2, soft2 = p.engine(_fs(), mfs, Pfs, S, normals=z, want_paths=False, select=dict(comp=-2, func='softplus'))
        assert none is None and nopaths is None and nopaths2 is None
        assert both.shape == (B, S, T, 4) and soft.shape == (B, S, T)
        figs = {'paths': rel(alone, want), 'softplus': rel(soft2, so.softplus(want[..., 2])), 'identity': rel(ident, want[..., 1])}
        print(f'{name} T={T} S={S}: ' + ' '.join(f'{k} {v:.2e}' for k, v in figs.items()) + f' (gate {gate:.1e})')
        assert np.array_equal(both, alone) and np.array_equal(soft, soft2)          # an output does not depend on which others are written
        assert max(figs.values()) <= gate, figs


@pytest.mark.parametrize('name', list(so.GPU_GATE))
def test_philox_stream_and_its_addressing(name):
    T, S, seed, trial0, sample0 = 130, 70, 77, 5, 3
    p, mfs, Pfs, maps = setup(name, T)
    got, comp = p.engine(_fs(), mfs, Pfs, S, seed=seed, trial0=trial0, sample0=sample0, select=dict(comp=2, func='softplus'))
    z = np.stack([so.philox_normals(seed, trial0 + b, range(sample0, sample0 + S), T, 4) for b in range(B)])
    want = oracle_paths(mfs, Pfs, maps, z)
    fig = rel(got, want)
    print(f'{name}: Philox stream vs oracle {fig:.2e} (gate {so.GPU_GATE[name] + so.BOX_MULLER:.1e})')
    assert fig <= so.GPU_GATE[name] + so.BOX_MULLER
    # one launch = six launches of one trial and 64 | 6 samples, bit for bit
    for b in range(B):
        for s0, n in ((0, 64), (64, 6)):
            part, cpart = p.engine(_fs(), mfs[b:b + 1], Pfs[b:b + 1], n, seed=seed, trial0=trial0 + b, sample0=sample0 + s0,
                                   select=dict(comp=2, func='softplus'))
            assert np.array_equal(part[0], got[b, s0:s0 + n]) and np.array_equal(cpart[0], comp[b, s0:s0 + n]), (b, s0)
    other, _ = p.engine(_fs(), mfs, Pfs, S, seed=seed + 1, trial0=trial0, sample0=sample0, select=dict(comp=2, func='softplus'))
    assert not np.array_equal(other, got)


def test_joint_law_of_the_chirp_model():
    T, S = 130, 4096
    p, mfs, Pfs, maps = setup('eks_chirp', T, 2)
    x, _ = p.engine(_fs(), mfs, Pfs, S, seed=STAT_SEED)
    mss_e, Pss_e = _fs().eks(p.case.disc, mfs, Pfs, p.case.dt)
    for b in range(2):
        mss, Pss, lag = so.smoother_moments(maps[b], mfs[b], Pfs[b])
        assert rel(mss_e[b], mss) <= 1e-9 and rel(Pss_e[b], Pss) <= 1e-9              # the moments compared with are the engine's smoother's
        ex = so.moment_excess(x[b], mss, Pss, lag)
        print('chirp joint law, trial', b, ex)
        assert max(ex.values()) <= STAT_GATE, ex


def test_lascala_zero_columns():
    T, S = 130, 4096
    name = 'eks_lascala'
    p, mfs, Pfs, maps = setup(name, T, 2)
    x, _ = p.engine(_fs(), mfs, Pfs, S, seed=STAT_SEED)
    assert np.isfinite(x).all()
    for b in range(2):
        G, c, _ = maps[b]
        det = c[None, :, :2] + np.einsum('tij,stj->sti', G[:, :2, :], x[b, :, 1:, :])    # c_t + G_t x_{t+1}, the chirp components
        fig = float(np.max(np.abs(x[b, :, :-1, :2] - det)) / np.max(np.abs(x[b])))
        print(f'La Scala trial {b}: chirp components vs c + G x {fig:.2e} of the largest entry (gate {so.GPU_GATE[name]:.1e})')
        assert fig <= so.GPU_GATE[name]
        mss, Pss, lag = so.smoother_moments(maps[b], mfs[b], Pfs[b])
        ex = so.moment_excess(x[b][..., 2:], mss[:, 2:], Pss[:, 2:, 2:], lag[:, 2:, 2:])
        print('La Scala M32 block, trial', b, ex)
        assert max(ex.values()) <= STAT_GATE, ex


def test_records_with_gaps_and_a_forecast_tail():
    T, S, tail = 130, 70, 100
    p = so.pairs()['eks_chirp']
    ys = np.stack([p.case.ys[:T] + 0.05 * b for b in range(B)])
    ys[:, 40:60] = np.nan
    ys[:, tail:] = np.nan
    mfs, Pfs = _filter(p, ys, missing='skip')
    assert np.isfinite(mfs).all() and np.isfinite(Pfs).all()
    maps = [so.oracle_maps(p, mfs[b], Pfs[b]) for b in range(B)]
    z = np.random.default_rng(5).standard_normal((B, S, T, 4))
    got, _ = p.engine(_fs(), mfs, Pfs, S, normals=z)
    fig = rel(got, oracle_paths(mfs, Pfs, maps, z))
    print(f'gaps: vs oracle {fig:.2e} (gate {so.GPU_GATE["eks_chirp"]:.1e})')
    assert fig <= so.GPU_GATE['eks_chirp']
    # the forecast ensemble: over the tail the variance of y = H x grows with the horizon
    S2 = 4096
    _, y = p.engine(_fs(), mfs[:1], Pfs[:1], S2, seed=STAT_SEED, want_paths=False, select=dict(comp=1, func='identity'))     # H = e_1
    assert np.array_equal(p.case.H, [0., 1., 0., 0.])
    _, Pss, _ = so.smoother_moments(maps[0], mfs[0], Pfs[0])
    assert (np.diff(Pss[tail:, 1, 1]) > 0).all()                                   # ... as the smoother's own does
    v = y[0].var(axis=0, ddof=1)[tail:]
    se = v * np.sqrt(2.0 / S2)                                                     # standard error of a variance estimate
    assert (v[1:] >= v[:-1] - STAT_GATE * se[1:]).all() and v[-1] > 2 * v[0], v


def test_nan_rows():
    T, S, t0 = 130, 70, 80
    p, mfs, Pfs, _ = setup('eks_chirp', T)
    mfs = np.array(mfs)
    mfs[1, t0, 2] = np.nan
    x, comp = p.engine(_fs(), mfs, Pfs, S, seed=1, select=dict(comp=2, func='softplus'))
    assert np.isnan(x[1, :, :t0 + 1]).all() and np.isfinite(x[1, :, t0 + 1:]).all()
    assert np.isnan(comp[1, :, :t0 + 1]).all() and np.isfinite(comp[1, :, t0 + 1:]).all()
    assert np.isfinite(x[0]).all() and np.isfinite(x[2]).all()


def _raw(method, spec, mfs, Pfs, S, paths=True, comp_paths=False, comp=0, func=0, flags=0):
    """The entry point itself, for the argument checks the Python layer makes first."""
    import torch
    from chirpgp_amd import _engine as E
    m, P = E.dev(mfs), E.dev(Pfs)
    nb, T, d = m.shape
    keep = []
    ctx = E.context(m.device.index)
    model = E._model_struct(spec, None, nb, keep)
    o = E.CgpSampleOut()
    out = torch.empty((nb, S, T, d), dtype=torch.float64, device=m.device)
    cout = torch.empty((nb, S, T), dtype=torch.float64, device=m.device)
    o.paths, o.comp_paths, o.comp, o.func = (E._ptr(out) if paths else None), (E._ptr(cout) if comp_paths else None), comp, func
    lib = E.load_library()
    rc = lib.cgp_smoother_sample(ctx, method, C.byref(model), None, float(1e-3), E._ptr(m), E._ptr(P), nb, T, S, 0, 0, 0, None, C.byref(o), flags, E._stream())
    torch.cuda.synchronize()
    return rc, lib.cgp_last_error(ctx).decode()


def test_arguments():
    from chirpgp_amd import _engine as E
    p, mfs, Pfs, _ = setup('eks_chirp', 2)
    spec = p.case.disc
    rc, msg = _raw(E.S_EKS, spec, mfs, Pfs, 4, flags=0x800)
    assert rc == -1 and 'CGP_TIME_SPLIT' in msg
    rc, msg = _raw(E.S_EKS, spec, mfs, Pfs, 4, paths=False)
    assert rc == -1 and 'both NULL' in msg
    for comp in (-1, 4):
        rc, msg = _raw(E.S_EKS, spec, mfs, Pfs, 4, comp_paths=True, comp=comp)
        assert rc == -1 and 'comp' in msg
    rc, msg = _raw(E.S_CD_EKS, spec, mfs, Pfs, 4)
    assert rc == -2 and 'continuous-discrete' in msg
    assert _raw(E.S_EKS, spec, mfs, Pfs, 0)[0] == 0                                    # S = 0: nothing to do
    for kw in (dict(trial0=2 ** 32 - 2), dict(sample0=2 ** 32 - 3)):                    # B = 3, S = 4: past the counter's words
        with pytest.raises(RuntimeError, match=r'2\^32'):
            p.engine(_fs(), mfs, Pfs, 4, **kw)
    x, _ = p.engine(_fs(), mfs, Pfs, 4, trial0=2 ** 32 - 3, sample0=2 ** 32 - 4)       # the last trials and samples there are
    assert np.isfinite(x).all()
    with pytest.raises(RuntimeError, match='CGP_WAVE_PER_TRIAL'):
        p.engine(_fs(), mfs, Pfs, 4, flags=0x2)
    empty, _ = p.engine(_fs(), mfs[:, :0], Pfs[:, :0], 4)
    assert empty.shape == (B, 4, 0, 4)
