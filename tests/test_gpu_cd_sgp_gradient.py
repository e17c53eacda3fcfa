"""cgp_sgp_nll_grad on the SDE model (csrc/cgp_tangent4_cd_sigma.hpp) -- the continuous-discrete sigma-point filter's final NLL and its
exact gradient, forward tangents through the Cholesky factor and the sigma-point sums of the four RK4 stages of every step -- against
values and gradients computed in 100-digit arithmetic (tests/golden/exact_cd_sgp_grad.npz, written by
tests/golden/make_exact_cd_sgp_grad.py), through the raw C-ABI and through mle.value_and_grad; against filters_smoothers.cd_sgp_filter for
the value; launch shapes and direction counts (one pass, slices), records with gaps, substeps, edge inputs, guard bands, the refusals on
the device, and the L-BFGS front ends with the demo.

Gates (tests/cd_sgp_grad_cases.py): value 1e-11 relative, gradient 1e-8 of its largest component -- the project's tangent-kernel gates --
and for the cases exempt from admission max(gate, 100 x the stored movement); bit-identity where two launches run the same trial.

RESULTS on an MI355X (printed by the tests; none of them set a gate).  Wall time of this file: 7 s for its 58 tests.
  * fixture cases: value <= 2.9e-15 (random_cds_01), gradient <= 6.7e-15 of its scale (substeps_cds_n4); record lengths: 1.5e-15 / 1.6e-15.
  * against filters_smoothers.cd_sgp_filter's final NLL: <= 1.3e-13.
  * n = 3 substeps against the flagged kernel on the refined record: the same bits, with gaps of its own and without.
  * the difference gradient of 13 batched_nll probes sits 4.4e-10 .. 9.6e-10 of the gradient's scale from the exact one.
  * fit(exact=True) on the T = 600 record (cubature): 131.8421626400415 in 36 iterations (40 launches); the difference route
    131.8421625009672 in 52 (60): 1.05e-9 apart.
  * on the parent commit every test here fails: cgp_sgp_nll_grad refuses the SDE model, _engine has no run_cd_sgp_nll_grad and mle no
    route for 'cd_sgp_filter'."""
import os
import subprocess
import sys

import numpy as np
import numpy.testing as npt
import pytest

from tests.cd_sgp_grad_cases import (ENTRY, GRAD_GATE, NAMES, PREFIX_NAMES, PREFIX_T, SKIP_MISSING, VALUE_RTOL, Z, builder, case, directions,
                                     errors, gates, raw, rk4_substeps, sigma_points)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 123.0
E_ARG, E_UNSUPPORTED = -1, -2


def _missing(c):
    return 'skip' if c['skip'] else None


def _flags(c):
    return (SKIP_MISSING if c['skip'] else 0) | rk4_substeps(c['n'])


def _vg(c, T=None, thetas=None, ys=None, sigma=None, **kw):
    """mle.value_and_grad(method='cd_sgp_filter') on a case (its first T measurements; other parameter vectors or records on request)."""
    from chirpgp_amd import mle
    ys = (c['ys'] if T is None else c['ys'][:T]) if ys is None else ys
    kw.setdefault('missing', _missing(c))
    kw.setdefault('substeps', c['n'])
    return mle.value_and_grad(builder(c['build']), c['theta'][None, :] if thetas is None else thetas, ys, c['Xi'], c['dt'], method='cd_sgp_filter',
                              sgps=sigma_points(sigma or c['sigma']), **kw)


def _run_dirs(c, dirs, thetas=None, ys=None, T=None, H=None, m0=None, P0=None, sigma=None, shared_model=False, **kw):
    """E.run_cd_sgp_nll_grad with the caller's directions (B, n_dir, 27) and, on request, its own H / m0 / P0, parameter vectors and
    records; shared_model: the drift's parameters and gamma of ONE vector for every trial (param_stride = gamma_stride = 0)."""
    from chirpgp_amd import _engine as E, models as pm
    thetas = c['theta'][None, :] if thetas is None else thetas
    with np.errstate(all='ignore'):
        drift, disp, _, m0_, P0_, _ = builder(c['build'])(pm.g(thetas[0] if shared_model else thetas))
    ys = (c['ys'] if T is None else c['ys'][:T]) if ys is None else ys
    kw.setdefault('missing', _missing(c))
    kw.setdefault('substeps', c['n'])
    out = E.run_cd_sgp_nll_grad(drift, disp.outer(), sigma_points(sigma or c['sigma']), c['H'] if H is None else H, c['Xi'], m0_ if m0 is None else m0,
                                P0_ if P0 is None else P0, c['dt'], ys, dirs, **kw)
    return tuple(o.cpu().numpy() for o in out)


# ------------------------------------------------------------------------------------------------ 1. every fixture case
@pytest.mark.parametrize('name', NAMES)
def test_fixture_case(name):
    """Every case through the raw C-ABI (output buffers pre-filled) and through mle.value_and_grad (other_cds_H_dXi: through the engine
    call, which takes its H and the seventh direction d Xi = 1): the same bits from both, within the gates of the 100-digit numbers.  The
    gapped cases run with CGP_SKIP_MISSING / missing='skip', the substeps cases with CGP_RK4_SUBSTEPS(n) / substeps=n; the record of NaN
    only gives exactly +0.0 and a zero gradient."""
    c = case(name)
    dirs = directions(c)
    rc, msg, nll, grad = raw(c, c['ys'].size, dirs[0], FILL, flags=_flags(c))
    assert rc == 0, msg
    if c['with_dxi']:
        f, g_ = _run_dirs(c, dirs)
    else:
        f, g_ = _vg(c)
    npt.assert_array_equal(f, nll)
    npt.assert_array_equal(g_, grad)
    value_gate, grad_gate = gates(c)
    ev, eg = errors(nll[0], grad[0], c['nll'], c['grad'], name)
    if c['group'] == 'edge':
        print(f'   moved by {c["moved_nll"]:.2e} / {c["moved_grad"]:.2e} under the 1e-15 perturbation -> gates {value_gate:.2e} / {grad_gate:.2e}')
    assert ev < value_gate, (nll[0], c['nll'])
    assert eg < grad_gate, (grad[0], c['grad'])
    if name == 'gaps_cds_everywhere':
        assert nll[0] == 0.0 and not np.signbit(nll[0]) and np.array_equal(grad[0], np.zeros(6))


# ------------------------------------------------------------------------------------------------ 2. record lengths
@pytest.mark.parametrize('name', PREFIX_NAMES)
def test_record_lengths(name):
    """Measurements are fetched 64 steps at a time: T = 1, 2, 63, 64, 65, 128, 129, 130 against the 100-digit value and gradient of every
    prefix of one record, with the cubature rule (8 points: the narrow reduction) and Gauss-Hermite order 3 (81: two points a lane)."""
    c = case(name)
    want_f, want_g = Z[f'{name}.nll_prefix'], Z[f'{name}.grad_prefix']
    dirs = directions(c)[0]
    worst = [0., 0.]
    for T in PREFIX_T:
        rc, msg, nll, grad = raw(c, T, dirs, FILL)
        assert rc == 0, msg
        ev, eg = errors(nll[0], grad[0], want_f[T - 1], want_g[T - 1], f'{name} T = {T}')
        worst = [max(worst[0], ev), max(worst[1], eg)]
        assert ev < VALUE_RTOL and eg < GRAD_GATE, (T, nll[0], want_f[T - 1], grad[0], want_g[T - 1])
    f, g_ = _vg(c, T=65)
    rc, msg, nll, grad = raw(c, 65, dirs, FILL)
    npt.assert_array_equal(f, nll)
    npt.assert_array_equal(g_, grad)
    print(f'{name}: worst over the record lengths: value {worst[0]:.2e}, gradient {worst[1]:.2e}')


def test_an_empty_record_writes_zeros():
    c = case('prefix_cds_cubature')
    for n_dir in (6, 17):                                     # (one launch; two slices)
        dirs = np.resize(directions(c)[0], (n_dir, 27))
        rc, msg, nll, grad = raw(c, 0, dirs, np.nan, B=2)
        assert rc == 0, msg
        assert np.array_equal(nll, [0.0, 0.0]) and np.array_equal(grad, np.zeros((2, n_dir)))
    f, g_ = _vg(c, ys=np.zeros(0))
    assert np.array_equal(f, [0.0]) and np.array_equal(g_, np.zeros((1, 6)))


# ------------------------------------------------------------------------------------------------ 3. the value is cd_sgp_filter's
def test_the_value_is_cd_sgp_filters_final_nll():
    """On every fixture case the value equals the final NLL of filters_smoothers.cd_sgp_filter on the same inputs to 1e-11 relative (the
    gapped cases with missing='skip' on both sides, the substeps cases with substeps=n; the record of NaN only: both exactly 0)."""
    from chirpgp_amd import filters_smoothers as fs, models as pm
    worst = 0.0
    for name in NAMES:
        c = case(name)
        drift, disp, _, m0, P0, _ = builder(c['build'])(pm.g(c['theta']))
        sub = dict(substeps=c['n']) if c['n'] != 1 else {}
        want = float(np.asarray(fs.cd_sgp_filter(drift, disp, sigma_points(c['sigma']), c['H'], c['Xi'], m0, P0, c['dt'], c['ys'], nll_final_only=True,
                                                 want=(False, False, True), missing=_missing(c), **sub)[2]).reshape(-1)[0])
        f, _ = _run_dirs(c, directions(c))
        err = abs(f[0] - want) / (abs(want) if want != 0 else 1.0)
        print(f'{name}: {f[0]!r} against cd_sgp_filter {want!r}: {err:.2e}')
        worst = max(worst, err)
        assert err < VALUE_RTOL, name
    print(f'worst: {worst:.2e}')


# ------------------------------------------------------------------------------------------------ 4. launch shapes and direction counts
def _chirp_thetas():
    rows = [Z['prefix_cds_cubature.theta']] + [Z[f'{n}.theta'] for n in NAMES if n.startswith('random_cds') and str(Z[f'{n}.build']) == 'chirp'
                                               and float(Z[f'{n}.dt']) == 1e-3]
    return np.stack(rows)


def _dirs_n(c, thetas, n_dir):
    """n_dir directions per trial: direction k is parameter direction k mod 7, the seventh being d Xi = 1."""
    d = directions(c, thetas)
    d7 = np.zeros((thetas.shape[0], 1, 27))
    d7[:, 0, 12] = 1.0
    d = np.concatenate([d, d7], axis=1)
    return np.ascontiguousarray(d[:, np.arange(n_dir) % 7])


T_SHAPES = 20


@pytest.fixture(scope='module')
def alone():
    """(sigma, n_dir) -> the 22 single-trial launches of the launch-shape tests, computed once."""
    cache = {}

    def get(sigma, n_dir):
        if (sigma, n_dir) not in cache:
            c = case('prefix_cds_cubature')
            pool = _chirp_thetas()
            thetas = pool[np.arange(22) % pool.shape[0]]
            cache[(sigma, n_dir)] = (thetas, [_run_dirs(c, _dirs_n(c, thetas[t:t + 1], n_dir), thetas=thetas[t:t + 1], T=T_SHAPES, sigma=sigma)
                                              for t in range(22)])
        return cache[(sigma, n_dir)]
    return get


@pytest.mark.parametrize('n_dir', [4, 6, 7])
def test_launch_shapes(n_dir, alone):
    """B = 1, 11 and 22, every trial with its own parameters and gamma (param_stride, gamma_stride) on one shared record (ys_repeat = B):
    every trial's row equals its single-trial launch bit for bit; trial 0 (the prefix case's parameters) within the gates."""
    c = case('prefix_cds_cubature')
    thetas, single = alone('cubature', n_dir)
    for B in (1, 11, 22):
        f, grad = _run_dirs(c, _dirs_n(c, thetas[:B], n_dir), thetas=thetas[:B], T=T_SHAPES, trials_per_record=B)
        assert f.shape == (B,) and grad.shape == (B, n_dir)
        for t in range(B):
            npt.assert_array_equal(f[t], single[t][0][0], err_msg=f'B = {B} trial {t}')
            npt.assert_array_equal(grad[t], single[t][1][0], err_msg=f'B = {B} trial {t}')
        m = min(n_dir, 6)
        want_f, want_g = Z['prefix_cds_cubature.nll_prefix'][T_SHAPES - 1], Z['prefix_cds_cubature.grad_prefix'][T_SHAPES - 1]
        assert abs(f[0] - want_f) / abs(want_f) < VALUE_RTOL
        assert np.abs(grad[0, :m] - want_g[:m]).max() / np.abs(want_g).max() < GRAD_GATE


@pytest.mark.parametrize('sigma', ['cubature', 'gh3'])
@pytest.mark.parametrize('n_dir', [1, 2, 16, 17])
def test_direction_counts(n_dir, sigma):
    """n_dir = 1 (one pass of the fan), 2, 16 (every owner lane, nine passes) and 17 (two launches, the second with one direction): every
    entry within the gate of the 100-digit gradient's entry k mod 7 (the seventh: d / d Xi, against the sixteen-direction launch's own),
    the value within its gate and the same bits whatever n_dir; three trials equal their single launches bit for bit."""
    c = case(f'prefix_cds_{sigma}')
    T = T_SHAPES
    want_f, want_g = Z[f'{c["name"]}.nll_prefix'][T - 1], Z[f'{c["name"]}.grad_prefix'][T - 1]
    thetas = np.repeat(c['theta'][None, :], 3, axis=0)
    thetas[1:] = _chirp_thetas()[1:3]
    f, grad = _run_dirs(c, _dirs_n(c, thetas, n_dir), thetas=thetas, T=T, trials_per_record=3)
    assert f.shape == (3,) and grad.shape == (3, n_dir) and np.isfinite(f).all() and np.isfinite(grad).all()
    for t in range(3):
        ft, gt = _run_dirs(c, _dirs_n(c, thetas[t:t + 1], n_dir), thetas=thetas[t:t + 1], T=T)
        npt.assert_array_equal(ft[0], f[t])
        npt.assert_array_equal(gt[0], grad[t])
    assert abs(f[0] - want_f) / abs(want_f) < VALUE_RTOL
    f6, _ = _run_dirs(c, _dirs_n(c, thetas[:1], 6), thetas=thetas[:1], T=T)
    assert f[0] == f6[0]                                      # the primal does not depend on how many directions ride along
    scale = np.abs(want_g).max()
    for k in range(n_dir):
        if k % 7 < 6:
            assert abs(grad[0, k] - want_g[k % 7]) / scale < GRAD_GATE, (k, grad[0, k], want_g[k % 7])
    if n_dir > 7:
        assert abs(grad[0, 6]) > 0 and abs(grad[0, 13] - grad[0, 6]) / scale < GRAD_GATE


def test_shared_model_indexed_records_and_per_trial_operands():
    """One parameter vector and one gamma for every trial (param_stride = gamma_stride = 0) with per-trial H, m0 and P0; and through mle
    three records picked and permuted by record_index (ys_index) with two parameter vectors each (ys_repeat = 2): bit-identical to the
    same trials launched one by one."""
    c = case('prefix_cds_cubature')
    B, T = 5, 30
    rng = np.random.default_rng(56)
    dirs = np.repeat(directions(c), B, axis=0)
    H = rng.uniform(-1.5, 1.5, size=(B, 4))
    m0 = rng.uniform(-1, 1, size=(B, 4)) + np.array([0., 0., 7., 0.])
    A = rng.uniform(-0.3, 0.3, size=(B, 4, 4))
    P0 = np.eye(4)[None] * rng.uniform(0.1, 1.0, size=(B, 4))[:, None, :] + A @ A.transpose(0, 2, 1)
    f, grad = _run_dirs(c, dirs, T=T, H=H, m0=m0, P0=P0, shared_model=True, trials_per_record=B)
    assert np.isfinite(f).all() and np.isfinite(grad).all() and len({float(v) for v in f}) == B
    for i in range(B):
        fi, gi = _run_dirs(c, dirs[i:i + 1], T=T, H=H[i], m0=m0[i], P0=P0[i], shared_model=True)
        npt.assert_array_equal(fi[0], f[i])
        npt.assert_array_equal(gi[0], grad[i])
    ys = c['ys'][:T]
    recs = np.stack([ys, ys[::-1].copy(), 0.7 * ys + 0.3 * rng.standard_normal(ys.size), 1.1 * ys])
    index = np.array([2, 0, 3, 0])
    thetas = np.resize(_chirp_thetas(), (8, 6))
    f, grad = _vg(c, thetas=thetas, ys=recs, record_index=index)
    assert f.shape == (8,) and grad.shape == (8, 6)
    for t in range(8):
        ft, gt = _vg(c, thetas=thetas[t:t + 1], ys=recs[index[t // 2]])
        npt.assert_array_equal(ft[0], f[t], err_msg=f'trial {t}')
        npt.assert_array_equal(gt[0], grad[t], err_msg=f'trial {t}')


# ------------------------------------------------------------------------------------------------ 5. records with gaps
def test_the_flag_on_a_gap_free_record_gives_the_unflagged_result():
    """(Two instantiations of the kernel: the same numbers to 1e-11 of their scale, not necessarily the same bits.)"""
    for name in PREFIX_NAMES:
        c = case(name)
        dirs = directions(c)[0]
        for T in (9, 130):
            rc0, _, nll0, grad0 = raw(c, T, dirs, FILL)
            rc1, _, nll1, grad1 = raw(c, T, dirs, FILL, flags=SKIP_MISSING)
            assert rc0 == 0 and rc1 == 0
            assert abs(nll1[0] - nll0[0]) <= 1e-11 * abs(nll0[0])
            assert np.abs(grad1 - grad0).max() <= 1e-11 * np.abs(grad0).max()


def test_trailing_gaps_add_nothing_and_a_record_of_nan_gives_zero():
    c = case('prefix_cds_cubature')
    ys = c['ys'][:50]
    f0, g0 = _vg(c, ys=ys, missing='skip')
    for tail in (1, 14, 15, 80):                              # to the end of the 64-step chunk, one past it, and a whole chunk more
        f1, g1 = _vg(c, ys=np.r_[ys, np.full(tail, np.nan)], missing='skip')
        npt.assert_array_equal(f1, f0)
        npt.assert_array_equal(g1, g0)
    for n_dir in (6, 17):
        dirs = np.resize(directions(c)[0], (1, n_dir, 27))
        f, g_ = _run_dirs(c, dirs, ys=np.full(70, np.nan), missing='skip')
        assert f[0] == 0.0 and not np.signbit(f[0]) and np.array_equal(g_, np.zeros((1, n_dir)))
    f, g_ = _vg(case('gaps_cds_run'), missing=None)           # without the flag a NaN measurement is what it is in the reference
    assert np.isnan(f).all() and np.isnan(g_).all()


def test_a_gapped_record_among_three_touches_its_trial_only():
    c, clean = case('gaps_cds_run'), case('prefix_cds_cubature')
    recs = np.stack([clean['ys'][:40], c['ys'], clean['ys'][:40][::-1].copy()])
    thetas = np.repeat(c['theta'][None, :], 3, axis=0)
    f, g_ = _vg(c, thetas=thetas, ys=recs, missing='skip')
    for t in (0, 2):
        ft, gt = _vg(clean, ys=recs[t], missing='skip')
        npt.assert_array_equal(ft[0], f[t])
        npt.assert_array_equal(gt[0], g_[t])
    ev, eg = errors(f[1], g_[1], c['nll'], c['grad'], 'the gapped record among three')
    assert ev < VALUE_RTOL and eg < GRAD_GATE


# ------------------------------------------------------------------------------------------------ 6. substeps
@pytest.mark.parametrize('name', PREFIX_NAMES)
def test_three_substeps_are_the_flagged_kernel_on_the_refined_record(name):
    """CGP_RK4_SUBSTEPS(3) against CGP_SKIP_MISSING on the three-times refined record (NaN at the inserted times) at dt / 3: the same
    recursion by definition (include/chirpgp_hip.h), at the fixture's gates; with gaps of its own as well."""
    from chirpgp_amd import mle
    c = case(name)
    T = 40
    for gaps in (False, True):
        ys = c['ys'][:T].copy()
        if gaps:
            ys[[0, 7, 8, 39]] = np.nan
        fine = np.full(3 * T, np.nan)
        fine[2::3] = ys
        f3, g3 = _vg(c, ys=ys, substeps=3, missing='skip' if gaps else None)
        f1, g1 = mle.value_and_grad(builder(c['build']), c['theta'][None, :], fine, c['Xi'], c['dt'] / 3, method='cd_sgp_filter', sgps=sigma_points(c['sigma']),
                                    missing='skip')
        ev, eg = errors(f3[0], g3[0], f1[0], g1[0], f'{name} n = 3{", gaps" if gaps else ""}')
        assert ev < VALUE_RTOL and eg < GRAD_GATE
        assert f3[0] != _vg(c, ys=ys, missing='skip' if gaps else None)[0][0]          # (the substeps do something)


# ------------------------------------------------------------------------------------------------ 7. edge inputs
def test_a_p0_that_is_not_positive_definite_is_nan_and_alone():
    """A deterministic input: P0 = diag(1, -1, 1, 1) for one trial of three gives NaN in that trial's value and in every entry of its
    gradient (n_dir = 6 and 17: both slices), the other two bit-identical to the clean launch."""
    from chirpgp_amd import models as pm
    c = case('prefix_cds_cubature')
    _, _, _, _, P0, _ = builder(c['build'])(pm.g(c['theta']))
    for n_dir in (6, 17):
        dirs = np.resize(directions(c), (1, n_dir, 27)).repeat(3, axis=0)
        P0s = np.repeat(np.asarray(P0)[None], 3, axis=0)
        clean_f, clean_g = _run_dirs(c, dirs, T=40, P0=P0s, shared_model=True, trials_per_record=3)
        assert np.isfinite(clean_f).all() and np.isfinite(clean_g).all()
        P0s[1] = np.diag([1.0, -1.0, 1.0, 1.0])
        f, grad = _run_dirs(c, dirs, T=40, P0=P0s, shared_model=True, trials_per_record=3)
        assert np.isnan(f[1]) and np.isnan(grad[1]).all(), (f, grad)
        npt.assert_array_equal(f[[0, 2]], clean_f[[0, 2]])
        npt.assert_array_equal(grad[[0, 2]], clean_g[[0, 2]])
    rc, msg, nll, g_ = raw(c, 40, directions(c)[0], FILL, P0=np.diag([1.0, -1.0, 1.0, 1.0]))
    assert rc == 0 and np.isnan(nll).all() and np.isnan(g_).all(), (rc, msg, nll, g_)


# ------------------------------------------------------------------------------------------------ 8. guard bands
@pytest.mark.parametrize('placement', ['aligned', 'odd'])
def test_guard_bands(placement):
    """nll [B] and grad [B][n_dir] are written in full and nothing beside them is touched (tests/guard_bands.py), for one pass, several
    passes and two slices, one trial and five, T = 1 and 65, with gaps and substeps."""
    from chirpgp_amd import _engine as E
    from tests.test_gpu_guard_bands import guarded, model_data, records, sigma_points as gb_sigma
    sg = gb_sigma('cub', 4)
    for B in (1, 5):
        for T, kw in ((1, {}), (65, {}), (9, dict(missing='skip', substeps=2))):
            m = model_data('chirp_sde1', B, per_trial=B > 1, seed=T)
            ys = records(B, T, seed=B)
            for n_dir in (1, 6, 17):
                dirs = 0.1 * np.random.default_rng(n_dir).standard_normal((B, n_dir, 27))

                def call(inp):
                    spec, H, Xi, m0, P0 = inp.model(m)
                    return E.run_cd_sgp_nll_grad(spec, m.gamma, sg, H, Xi, m0, P0, m.dt, inp(ys, 'ys'), inp(dirs, 'dirs'), **kw)
                guarded(call, placement, False, ['nll', 'grad'], ('cd_sgp_nll_grad', B, T, n_dir))


# ------------------------------------------------------------------------------------------------ 9. the refusals, on the device
def test_refusals_leave_the_outputs_alone():
    c = case('prefix_cds_cubature')
    dirs = directions(c)[0]
    faults = [('gamma = NULL', lambda a: setattr(a['model'], 'gamma', None), E_UNSUPPORTED, b'model.gamma'),
              ('gamma_stride = 1', lambda a: setattr(a['model'], 'gamma_stride', 1), E_ARG, b'gamma_stride'),
              ('a d = 6 SDE model', lambda a: (setattr(a['model'], 'd', 6), setattr(a['model'], 'n_harm', 2)), E_UNSUPPORTED, b'n_harm = 1'),
              ('a stray flag beside the substeps', lambda a: a.update(flags=rk4_substeps(2) | 0x2), E_ARG, b'CGP_WAVE_PER_TRIAL'),
              ('dirs = NULL', lambda a: a.update(dirs=None), E_ARG, b'dirs')]
    for label, edit, code, word in faults:
        rc, msg, nll, grad = raw(c, 8, dirs, FILL, edit=edit)
        print(f'{ENTRY}, {label}: {rc} {msg.decode() if msg else ""}')
        assert rc == code and word in msg, (label, rc, msg)
        npt.assert_array_equal(nll, FILL, err_msg=label)
        npt.assert_array_equal(grad, FILL, err_msg=label)
    rc, msg, nll, grad = raw(c, 8, dirs, FILL, entry='cgp_sgp_nll_fisher')
    assert rc == E_UNSUPPORTED and b'Fisher form of the continuous-discrete filters is not built' in msg, (rc, msg)
    npt.assert_array_equal(nll, FILL)
    npt.assert_array_equal(grad, FILL)


# ------------------------------------------------------------------------------------------------ 10. mle and the demo
def test_value_and_grad_against_central_differences_of_batched_nll():
    """The route the kernel replaces: 13 probes of batched_nll, central differences with a relative step of 1e-6 -- within 1e-5 of the
    gradient's scale of the exact one (the differences' own error), with both sets, with gaps and with substeps."""
    from chirpgp_amd import mle
    for name, kw in (('prefix_cds_cubature', {}), ('prefix_cds_gh3', {}), ('gaps_cds_run', dict(missing='skip')), ('substeps_cds_n2', dict(substeps=2))):
        c = case(name)
        build, sg, theta = builder(c['build']), sigma_points(c['sigma']), c['theta']
        f, g_ = mle.value_and_grad(build, theta[None, :], c['ys'], c['Xi'], c['dt'], method='cd_sgp_filter', sgps=sg, **kw)
        P = theta.size
        h = 1e-6 * (1.0 + np.abs(theta))
        batch = np.tile(theta, (2 * P + 1, 1))
        for i in range(P):
            batch[1 + 2 * i, i] += h[i]
            batch[2 + 2 * i, i] -= h[i]
        nll = mle.batched_nll('cd_sgp_filter', build, batch, c['ys'], c['Xi'], c['dt'], sg, **kw)
        gd = (nll[1::2] - nll[2::2]) / (2 * h)
        err = np.abs(gd - g_[0]).max() / np.abs(g_[0]).max()
        print(f'{name}: the difference gradient is {err:.2e} of the scale from the exact one; values {abs(nll[0] - f[0]) / abs(f[0]):.2e} apart')
        assert abs(nll[0] - f[0]) <= 1e-11 * abs(f[0])
        assert err < 1e-5


def test_make_objective_and_fit_with_the_exact_gradient():
    """make_objective('cd_sgp_filter', exact=True) returns value_and_grad's numbers; exact=None stays the difference route; fit(exact=True)
    on the T = 600 record of tests/test_gpu_mle_oracle.py ends within that test's 1e-6 relative of the NLL the default difference-gradient
    fit reaches from the same start; fit_many(exact=True) takes the same route."""
    from chirpgp_amd import mle, models as pm
    from tests.test_gpu_mle_oracle import INIT, _record
    sg = sigma_points('cubature')
    ys = _record(600, 556)
    theta = pm.g_inv(INIT)
    fun = mle.make_objective('cd_sgp_filter', pm.build_chirp_model, ys, 0.1, 1e-3, sg, exact=True)
    f, g_ = fun(theta)
    vf, vg = mle.value_and_grad(pm.build_chirp_model, theta[None, :], ys, 0.1, 1e-3, method='cd_sgp_filter', sgps=sg)
    assert f == vf[0] and np.array_equal(g_, vg[0])
    fd, gd = mle.make_objective('cd_sgp_filter', pm.build_chirp_model, ys, 0.1, 1e-3, sg)(theta)            # exact=None: 13 probes
    assert abs(fd - f) <= 1e-11 * abs(f) and not np.array_equal(gd, g_)
    npt.assert_allclose(gd, g_, rtol=0, atol=1e-5 * np.abs(g_).max())
    opt, res = mle.fit('cd_sgp_filter', pm.build_chirp_model, INIT, ys, 0.1, 1e-3, sgps=sg, exact=True)
    opt_d, res_d = mle.fit('cd_sgp_filter', pm.build_chirp_model, INIT, ys, 0.1, 1e-3, sgps=sg)
    print(f'fit exact: nll {res.fun!r} in {res.nit} iterations ({res.nfev} launches); differences: {res_d.fun!r} in {res_d.nit} ({res_d.nfev}); '
          f'relative distance {abs(res.fun - res_d.fun) / abs(res_d.fun):.2e}')
    assert abs(res.fun - res_d.fun) <= 1e-6 * abs(res_d.fun), (res.fun, res_d.fun)
    start, _ = mle.value_and_grad(pm.build_chirp_model, theta[None, :], ys[:200], 0.1, 1e-3, method='cd_sgp_filter', sgps=sg)
    many, info = mle.fit_many('cd_sgp_filter', pm.build_chirp_model, INIT, ys[None, :200], 0.1, 1e-3, sgps=sg, maxiter=3, exact=True)
    assert np.isfinite(info['fun']).all() and info['fun'][0] < start[0] and info['nit'][0] >= 1


def test_the_demo_runs_with_the_exact_gradient():
    """demos/cd_ghfs_mle.py --exact on a short record, a few iterations, in a process of its own: it fits, filters, smooths and reports."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'demos', 'cd_ghfs_mle.py'), '--exact', '--T', '300', '--maxiter', '3'],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('cd_ghfs')]
    assert len(lines) == 3 and all('RMSE' in ln and 'nan' not in ln.lower() for ln in lines), out.stdout
