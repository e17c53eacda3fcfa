"""GPU tests of the posterior Cramer-Rao sums (cgp_pcrlb_sums) and the initial samples (cgp_simulate_x0).

Gate of the sums against the float64 oracle (tests/pcrlb_oracle.py): 10 x the oracle's own recorded distance from 100-digit arithmetic
(pcrlb_oracle.kernel_gate, per model), as max |difference| / the array's largest entry, for the D11 rows and the D12 rows separately.
The harmonic models run with the fixture's parameters, so that the figure was measured on the same Sigma; the linear models take the
d = 2 Matern model's figure and a well-conditioned Sigma.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import numpy.testing as npt
import pytest

from tests import guard_bands as gb
from tests import pcrlb_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (3, 2), (5, 63), (4, 64), (4, 65), (513, 130), (1030, 7))
MODELS = ('chirp', 'nh2', 'nh3', 'lin2', 'lin4', 'lin5')
_cache = {}


def exact():
    if 'exact' not in _cache:
        with np.load(os.path.join(ROOT, 'tests', 'golden', 'exact_pcrlb.npz')) as z:
            _cache['exact'] = {k: z[k] for k in z.files}
    return _cache['exact']


def model(name):
    """-> dict(spec, id, d, params, dt, m0, P0, H, Xi, gate): the harmonic models of the fixture; linear d = 2 (the fixture's), 4, 5."""
    if name in _cache:
        return _cache[name]
    from chirpgp_amd import models as M
    z = exact()
    if name in ('chirp', 'nh2', 'nh3'):
        d, p, dt = int(z[f'{name}_d']), z[f'{name}_params'], float(z[f'{name}_dt'])
        nh = (d - 2) // 2
        spec = M.disc_harmonic_chirp_lcd(p[0], p[1], p[2], p[3], nh, p[4])
        _, _, m0, P0, H = M.model_harmonic_chirp(p[0], p[1], p[2], p[3], 0.3, nh, p[4])
        out = dict(spec=spec, id=O.M_HARMONIC_LCD, d=d, params=p, dt=dt, m0=m0, P0=P0, H=H, Xi=0.1, gate=O.kernel_gate(name))
    else:
        d = int(name[3:])
        if d == 2:
            p = z['m32_params']
            F, S = p[:4].reshape(2, 2), p[4:].reshape(2, 2)
        else:
            rng = np.random.default_rng(d)
            F = 0.7 * np.eye(d) + 0.15 * rng.standard_normal((d, d))
            A = rng.standard_normal((d, d))
            S = 0.5 * np.eye(d) + 0.1 * A @ A.T
        spec = M.linear_cond_m_cov(F, S)
        out = dict(spec=spec, id=O.M_LINEAR, d=d, params=np.concatenate([F.ravel(), S.ravel()]), dt=0.1, m0=np.zeros(d), P0=np.eye(d) + 0.2,
                   H=np.eye(d)[0], Xi=0.1, gate=O.kernel_gate('m32'))
    _cache[name] = out
    return out


def states(m, B, T, key=5):
    from chirpgp_amd import tools
    xs, ys = tools.simulate_measurements(m['spec'], m['H'], m['Xi'], m['m0'], m['P0'], m['dt'], T, key, batch=B)
    return tools.simulate_initial(m['m0'], m['P0'], key, B), xs, ys


def figures(got, want, d):
    """max |difference| / largest entry, of the D11 rows and of the D12 rows."""
    n11 = d * (d + 1) // 2
    got, want = np.asarray(got), np.asarray(want)
    return tuple(float(np.max(np.abs(got[r] - want[r])) / np.max(np.abs(want[r]))) for r in (slice(0, n11), slice(n11, None)))


def check(got, want, m, what):
    f = figures(got, want, m['d'])
    print(what, f'D11 {f[0]:.2e}  D12 {f[1]:.2e}  gate {m["gate"]:.0e}')
    assert np.all(np.isfinite(got)), what
    assert max(f) <= m['gate'], (what, f)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'B{s[0]}-T{s[1]}')
@pytest.mark.parametrize('name', MODELS)
def test_sums_against_the_oracle(name, shape):
    """One step, both sides of the 64-step tile, both sides of a slab of 512 trials, ragged everything."""
    from chirpgp_amd import crlb
    m, (B, T) = model(name), shape
    x0, xs, _ = states(m, B, T)
    got = crlb.sums(m['spec'], m['dt'], x0, xs)
    assert tuple(got.shape) == (m['d'] * (m['d'] + 1) // 2 + m['d'] ** 2, T)
    check(got.cpu().numpy(), O.sums(m['id'], m['d'], m['params'], m['dt'], x0.cpu().numpy(), xs.cpu().numpy()), m, (name, shape))


@pytest.mark.parametrize('name', ('chirp', 'nh2', 'nh3', 'm32'))
def test_the_fixtures_hand_placed_pairs(name):
    """The fixture's pairs (the frequency state at -40, -1.75, -1.5, 0, 1.5, 2, 30, 650; one pair with r = 0) as T = 1 launches of one
    trial each, against the oracle's per-pair blocks; and all sixteen as one launch."""
    from chirpgp_amd import crlb
    z = exact()
    m = model({'m32': 'lin2'}.get(name, name))
    xs, xt = z[f'{name}_xs'], z[f'{name}_xt']
    want = O.pack(*O.pair_blocks(m['id'], m['d'], m['params'], m['dt'], xs, xt))                    # (16, K)
    got = np.stack([crlb.sums(m['spec'], m['dt'], xs[i:i + 1], xt[i:i + 1, None, :]).cpu().numpy()[:, 0] for i in range(len(xs))])
    check(got.T, want.T, m, (name, 'pair by pair'))
    check(crlb.sums(m['spec'], m['dt'], xs, xt[:, None, :]).cpu().numpy(), want.sum(axis=0)[:, None], m, (name, 'one launch'))
    # and against the 100-digit blocks themselves: the kernel's gate plus the oracle's own distance
    f = figures(got.T, O.pack(z[f'{name}_b11'], z[f'{name}_b12']).T, m['d'])
    assert max(f) <= 1.1 * m['gate'], f


def test_simulate_x0_is_the_simulators_initial_draw():
    import oracle.np_sim as ns
    from chirpgp_amd import _engine as E, tools
    from chirpgp_amd import models as M
    for d in (1, 2, 3, 4, 5, 8):
        rng = np.random.default_rng(d)
        A = rng.standard_normal((d, d))
        m0, P0 = rng.standard_normal(d), 0.3 * np.eye(d) + 0.2 * A @ A.T
        got = tools.simulate_initial(m0, P0, 9, 12).cpu().numpy()
        L0 = ns._chol(P0)
        want = np.stack([m0 + L0 @ ns._normals(9, tr, 0, d, ns.STREAM_INIT) for tr in range(12)])
        npt.assert_allclose(got, want, rtol=1e-11, atol=1e-11)
        # a shard equals the rows of the whole, bit for bit
        shard = tools.simulate_initial(m0, P0, 9, 5, trial0=7).cpu().numpy()
        assert np.array_equal(shard, got[7:12])
        # consistent with cgp_simulate: with F = I / 2 and (almost) no noise, x_1 = x_0 / 2
        xs = tools.simulate_sde(M.linear_cond_m_cov(0.5 * np.eye(d), 1e-30 * np.eye(d)), m0, P0, 0.1, 1, 9, batch=12).cpu().numpy()
        npt.assert_allclose(2 * xs[:, 0], got, rtol=0, atol=1e-14 * max(1.0, np.max(np.abs(got))))
    with pytest.raises(NotImplementedError):
        E.run_simulate_x0(9, np.zeros(9), np.eye(9), 1, 2)


def test_sums_accumulate():
    """A pre-filled buffer ends at 3 + sums; two half-batch calls agree with one call to the gate -- not bit for bit: the halves cut the
    slabs of 512 trials elsewhere, so the partial sums are other numbers added in another order."""
    import torch
    from chirpgp_amd import crlb
    m = model('chirp')
    x0, xs, _ = states(m, 1030, 70)
    one = crlb.sums(m['spec'], m['dt'], x0, xs)
    buf = torch.full_like(one, 3.0)
    out = crlb.sums(m['spec'], m['dt'], x0, xs, sums=buf)
    assert out.data_ptr() == buf.data_ptr()
    check(buf.cpu().numpy() - 3.0, one.cpu().numpy(), m, 'pre-filled')
    two = crlb.sums(m['spec'], m['dt'], x0[:500], xs[:500])
    crlb.sums(m['spec'], m['dt'], x0[500:], xs[500:], sums=two)
    check(two.cpu().numpy(), one.cpu().numpy(), m, 'two halves')
    with pytest.raises(ValueError, match='sums must be'):
        crlb.sums(m['spec'], m['dt'], x0, xs, sums=buf[:, :69])
    with pytest.raises(ValueError, match='sums must be'):
        crlb.sums(m['spec'], m['dt'], x0, xs, sums=buf.to(torch.float32))
    with pytest.raises(ValueError, match='xs must be'):
        crlb.sums(m['spec'], m['dt'], x0[:5], xs)


@pytest.mark.parametrize('nh', (1, 2))
def test_zero_frequency_scale_is_the_linear_model(nh):
    """freq_scale = 0: theta = 0 for every state, the model is x -> (rho I (+) M) x, and the second-order term vanishes."""
    from chirpgp_amd import crlb, models as M
    name = 'chirp' if nh == 1 else 'nh2'
    m = model(name)
    p, d = m['params'], m['d']
    spec0 = M.disc_harmonic_chirp_lcd(p[0], p[1], p[2], p[3], nh, 0.0)
    x0, xs, _ = states(m, 37, 66)
    F = np.zeros((d, d))
    F[np.arange(d - 2), np.arange(d - 2)] = np.exp(-p[0] * m['dt'])
    F[d - 2:, d - 2:] = O._m32(p[2], p[3], m['dt'])[0]
    lin = M.linear_cond_m_cov(F, O.sigma_of(O.M_HARMONIC_LCD, d, p, m['dt']))
    check(crlb.sums(spec0, m['dt'], x0, xs).cpu().numpy(), crlb.sums(lin, m['dt'], x0, xs).cpu().numpy(), m, ('freq_scale = 0', nh))


def test_reference_lgssm_test_on_the_device():
    """test/test_crlb.py:21-37, 75-87 with N = 4096: for a linear Gaussian model the bound is the Kalman filter's covariance, which is the
    same for every trial."""
    from chirpgp_amd import filters_smoothers as fs, models as M, tools
    ell, sigma, dt, T, N = 1., 1., 0.1, 10, 4096
    A = np.array([[0., 1.], [-3 / ell ** 2, -2 * np.sqrt(3) / ell]])
    Bv = np.array([0., 2 * sigma * (np.sqrt(3) / ell) ** 1.5])
    F, Sigma = tools.lti_sde_to_disc(A, Bv, dt)
    Xi, H = 1., np.array([1., 0.])
    m0, P0 = np.zeros(2), np.diag([sigma ** 2, 3 / ell ** 2 * sigma ** 2])
    spec = M.linear_cond_m_cov(F, Sigma)
    xs, ys = tools.simulate_measurements(spec, H, Xi, m0, P0, dt, T, 666, batch=N)
    x0 = tools.simulate_initial(m0, P0, 666, N)
    _, Pfs, _ = fs.kf(F, Sigma, H, Xi, m0, P0, ys)
    Pfs = Pfs.cpu().numpy()
    assert np.array_equal(Pfs, np.broadcast_to(Pfs[0], Pfs.shape))
    import torch
    xss = torch.cat([x0[:, None, :], xs], dim=1).transpose(0, 1)                      # (T + 1, N, d), time-major as the reference's
    js = M.posterior_cramer_rao(xss, ys.transpose(0, 1), np.linalg.inv(P0), spec, H, Xi, dt)
    assert js.shape == (T, 2, 2)
    npt.assert_allclose(np.linalg.inv(js), Pfs[0], atol=1e-12)
    # NumPy arrays in the reference's layout take the same way
    js_np = M.posterior_cramer_rao(xss.cpu().numpy(), ys.cpu().numpy().T, np.linalg.inv(P0), spec, H, Xi, dt)
    npt.assert_allclose(js_np, js, rtol=1e-13)


def test_nan_placement_and_broken_cholesky():
    """A NaN in xs[b][t] makes every row of steps t and t + 1 NaN and no other step; a Sigma whose Cholesky breaks (b = 0) makes all NaN."""
    from chirpgp_amd import crlb, models as M
    for name in ('chirp', 'lin4', 'nh3'):
        m = model(name)
        x0, xs, _ = states(m, 6, 130)
        clean = crlb.sums(m['spec'], m['dt'], x0, xs).cpu().numpy()
        bad = xs.clone()
        hits = ((2, 5, 0), (0, 63, m['d'] - 1), (5, 129, 1), (3, 100, m['d'] - 2))
        for b, t, i in hits:
            bad[b, t, i] = float('nan')
        got = crlb.sums(m['spec'], m['dt'], x0, bad).cpu().numpy()
        nan_steps = sorted({t for _, t, _ in hits} | {t + 1 for _, t, _ in hits if t + 1 < 130})
        assert np.all(np.isnan(got[:, nan_steps]))
        rest = np.setdiff1d(np.arange(130), nan_steps)
        assert np.array_equal(got[:, rest], clean[:, rest])                  # one slab: the same partial sums in the same order
        x0b = x0.clone()
        x0b[1, 0] = float('inf')
        got = crlb.sums(m['spec'], m['dt'], x0b, xs).cpu().numpy()
        assert np.all(np.isnan(got[:, 0])) and np.array_equal(got[:, 1:], clean[:, 1:])
    m = model('chirp')
    p = m['params']
    x0, xs, _ = states(m, 5, 7)
    assert np.all(np.isnan(crlb.sums(M.disc_chirp_lcd(p[0], 0.0, p[2], p[3]), m['dt'], x0, xs).cpu().numpy()))
    lin = model('lin2')
    S = lin['params'][4:].reshape(2, 2).copy()
    S[1, 1] = S[0, 1] ** 2 / S[0, 0] * 0.5                                       # not positive definite
    x0, xs, _ = states(lin, 5, 7)
    assert np.all(np.isnan(crlb.sums(M.linear_cond_m_cov(lin['params'][:4].reshape(2, 2), S), lin['dt'], x0, xs).cpu().numpy()))


def test_argument_table():
    """Section 2 of the header comment of cgp_pcrlb_sums / cgp_simulate_x0, code by code, with the messages."""
    import torch
    from chirpgp_amd import _engine as E, models as M
    lib, ctx = E.load_library(), E.context()
    m = model('chirp')
    x0, xs, _ = states(m, 3, 4)
    sums = torch.full((26, 4), 3.0, dtype=torch.float64, device='cuda')
    keep = []
    st = E._stream()

    def call(spec=m['spec'], x0=x0, xs=xs, B=3, T=4, sums=sums, flags=0, stride=None, null_model=False):
        ms = E._model_struct(spec, None, 1, keep)
        if stride is not None:
            ms.param_stride = stride
        rc = lib.cgp_pcrlb_sums(ctx, None if null_model else C.byref(ms), 0.01, E._ptr(x0), E._ptr(xs), B, T, E._ptr(sums), flags, st)
        return rc, (lib.cgp_last_error(ctx) or b'').decode()

    for bit, flag in ((E.NLL_FINAL_ONLY, 'CGP_NLL_FINAL_ONLY'), (E.WAVE_PER_TRIAL, 'CGP_WAVE_PER_TRIAL'), (E.SKIP_MISSING, 'CGP_SKIP_MISSING'),
                      (E.SIM_FIXED_X0, 'CGP_SIM_FIXED_X0')):
        rc, msg = call(flags=bit)
        assert rc == -1 and flag in msg and 'cgp_pcrlb_sums' in msg, msg
    for kw in (dict(x0=None), dict(xs=None), dict(sums=None)):
        rc, msg = call(**kw)
        assert rc == -1 and 'NULL' in msg, msg
    rc, msg = call(null_model=True)
    assert rc == -1 and 'NULL' in msg
    rc, msg = call(B=-1)
    assert rc == -1 and 'negative' in msg
    rc, msg = call(stride=5)
    assert rc == -1 and 'param_stride' in msg, msg
    rc, msg = call(spec=M.disc_model_lascala_lcd(1., 1.))
    assert rc == -2 and 'singular' in msg, msg
    drift = M.model_chirp(0.1, 0.1, 1., 1., 0.1)[0]
    lin_sde = M.linear_sde(-np.eye(4), np.ones(4))[0]
    for spec in (drift, lin_sde):
        rc, msg = call(spec=spec)
        assert rc == -2 and 'CGP_M_LINEAR and CGP_M_HARMONIC_LCD' in msg, msg
    kpt = M.DiscreteModel(E.M_KPT, 4, 2, np.zeros(32))
    rc, msg = call(spec=kpt)
    assert rc == -2, msg
    rc, msg = call(spec=M.disc_harmonic_chirp_lcd(0.1, 0.1, 1., 1., 4))         # d = 10: the filters have it, these sums do not
    assert rc == -2 and 'd <= 8' in msg, msg
    for kw in (dict(B=0), dict(T=0)):
        rc, _ = call(**kw)
        assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(sums == 3.0)                                               # nothing above wrote anything
    rc, _ = call()
    assert rc == 0
    torch.cuda.synchronize()
    assert not torch.any(sums[0] == 3.0)                                        # row 0, D11's (0, 0): trials x rho^2 / q

    # cgp_simulate_x0
    out = torch.full((3, 4), 3.0, dtype=torch.float64, device='cuda')
    init = E._init_struct(None, None, m['m0'], m['P0'], 4, 3, keep)
    ms = E._model_struct(m['spec'], None, 1, keep)
    assert lib.cgp_simulate_x0(ctx, C.byref(ms), None, 1, 0, 3, E._ptr(out), st) == -1 and b'init' in lib.cgp_last_error(ctx)
    assert lib.cgp_simulate_x0(ctx, None, C.byref(init), 1, 0, 3, E._ptr(out), st) == -1 and b'model' in lib.cgp_last_error(ctx)
    assert lib.cgp_simulate_x0(ctx, C.byref(ms), C.byref(init), 1, 0, 3, None, st) == -1 and b'x0' in lib.cgp_last_error(ctx)
    assert lib.cgp_simulate_x0(ctx, C.byref(ms), C.byref(init), 1, -1, 3, E._ptr(out), st) == -1
    ms.d = 9
    assert lib.cgp_simulate_x0(ctx, C.byref(ms), C.byref(init), 1, 0, 3, E._ptr(out), st) == -2 and b'1..8' in lib.cgp_last_error(ctx)
    ms.d = 4
    assert lib.cgp_simulate_x0(ctx, C.byref(ms), C.byref(init), 1, 0, 0, E._ptr(out), st) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 3.0)
    # the Python layer: one model per call
    with pytest.raises(ValueError):
        E.run_pcrlb_sums(M.disc_chirp_lcd(np.array([0.1, 0.2, 0.3]), 0.1, 1., 1.), 0.01, x0, xs)


@pytest.mark.parametrize('placement', gb.PLACEMENTS)
def test_guard_bands(placement):
    """sums and x0 are written in full and nothing beside them; the inputs are untouched (their guards hold NaN: a read beyond an input shows
    in the sums)."""
    from chirpgp_amd import _engine as E, tools
    for name, B, T in (('chirp', 1, 1), ('chirp', 5, 65), ('nh3', 515, 3), ('lin5', 66, 64), ('lin2', 3, 130)):
        m = model(name)
        x0, xs, _ = states(m, B, T)
        arena = gb.Arena('cuda', placement)
        gx0, gxs = arena.input(x0, 'x0'), arena.input(xs, 'xs')
        with arena.installed():
            got = E.run_pcrlb_sums(m['spec'], m['dt'], gx0, gxs)
        assert arena.check() == [], (name, B, T)
        assert gb.same_bits(gx0, x0) and gb.same_bits(gxs, xs)
        check(got.cpu().numpy(), E.run_pcrlb_sums(m['spec'], m['dt'], x0, xs).cpu().numpy(), m, ('guarded', name, B, T))
        arena = gb.Arena('cuda', placement)
        gm0, gP0 = arena.input(m['m0'], 'm0'), arena.input(m['P0'], 'P0')
        with arena.installed():
            g0 = tools.simulate_initial(gm0, gP0, 5, B)
        assert arena.check() == [], (name, B)
        assert gb.same_bits(g0, x0)


def test_demo_runs(tmp_path):
    """demos/crlb_model.py --num-mcs 4096 --T 20 --with-ekf --save: shapes, symmetry of js to 1e-10 of its scale, a positive diagonal of the
    bound, and the three report lines."""
    out = tmp_path / 'bound.npz'
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'demos', 'crlb_model.py'), '--num-mcs', '4096', '--T', '20', '--chunk', '3000',
                          '--with-ekf', '--save', str(out)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    with np.load(out) as z:
        ts, js, cc, cv = z['ts'], z['js'], z['crlb_chirps'], z['crlb_vs']
    assert ts.shape == (20,) and js.shape == (20, 4, 4) and cc.shape == (20,) and cv.shape == (20,)
    assert np.all(np.isfinite(js))
    asym = np.max(np.abs(js - np.swapaxes(js, 1, 2))) / np.max(np.abs(js))
    print(f'asymmetry of js / its scale: {asym:.2e}')
    assert asym <= 1e-10
    assert np.all(cc > 0) and np.all(cv > 0)
    assert np.all(np.diagonal(np.linalg.inv(js), axis1=1, axis2=2) > 0)
    lines = [ln for ln in run.stdout.splitlines() if 'bound / EKF MSE' in ln]
    assert len(lines) == 3, run.stdout
