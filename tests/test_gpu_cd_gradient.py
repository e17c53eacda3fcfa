"""cgp_cd_ekf_nll_grad (csrc/cgp_tangent4_cd.hpp) -- the continuous-discrete EKF's final NLL and its exact gradient, forward tangents
through the four RK4 stages of every step -- against values and gradients computed in 100-digit arithmetic
(tests/golden/exact_cd_grad.npz, written by tests/golden/make_exact_cd_grad.py), through the raw C-ABI and through mle.value_and_grad;
against filters_smoothers.cd_ekf for the value; launch shapes, per-trial operands, shared and indexed records, a diverged trial, the
argument table, records with gaps, and the L-BFGS front ends.

Gates (tests/cd_grad_cases.py): value 1e-11 relative, gradient 1e-8 of its largest component -- the discrete tangent kernels' -- and for
the cases exempt from admission max(gate, 100 x the stored movement); bit-identity where two launches run the same trial.

RESULTS on an MI355X (printed by the tests; none of them set a gate).  Wall time of this file: 3 s for its 41 tests.
  * fixture cases: value <= 2.0e-15 (random_cd_14), gradient <= 1.5e-14 of its scale (random_cd_11); record lengths: 1.0e-15 / 7.0e-15.
  * against filters_smoothers.cd_ekf's final NLL: <= 2.3e-12 (random_cd_14).
  * fit(exact=True) on the T = 600 record: 130.5447792896982 in 35 iterations (41 launches); the difference route 130.54477836353564 in
    53 (62): 7.1e-9 apart.
  * on the parent commit every test here fails: the symbol and the method do not exist there."""
import numpy as np
import numpy.testing as npt
import pytest

from tests.cd_grad_cases import ENTRY, GRAD_GATE, NAMES, PREFIX_T, SKIP_MISSING, VALUE_RTOL, Z, builder, case, directions, errors, gates, raw

pytestmark = pytest.mark.gpu
FILL = 123.0
E_ARG, E_UNSUPPORTED = -1, -2


def _missing(c):
    return 'skip' if c['skip'] else None


def _vg(c, T=None, thetas=None, ys=None, **kw):
    """mle.value_and_grad(method='cd_ekf') on a case (its first T measurements; other parameter vectors or records on request)."""
    from chirpgp_amd import mle
    ys = (c['ys'] if T is None else c['ys'][:T]) if ys is None else ys
    kw.setdefault('missing', _missing(c))
    return mle.value_and_grad(builder(c['build']), c['theta'][None, :] if thetas is None else thetas, ys, c['Xi'], c['dt'], method='cd_ekf', **kw)


def _run_dirs(c, dirs, thetas=None, ys=None, T=None, H=None, m0=None, P0=None, gamma=None, shared_model=False, **kw):
    """E.run_cd_ekf_nll_grad with the caller's directions (B, n_dir, 27) and, on request, its own H / m0 / P0 / gamma, parameter vectors
    and records; shared_model: the drift's parameters and gamma of ONE vector for every trial (param_stride = gamma_stride = 0)."""
    from chirpgp_amd import _engine as E, models as pm
    thetas = c['theta'][None, :] if thetas is None else thetas
    with np.errstate(all='ignore'):
        drift, disp, _, m0_, P0_, _ = builder(c['build'])(pm.g(thetas[0] if shared_model else thetas))
    ys = (c['ys'] if T is None else c['ys'][:T]) if ys is None else ys
    kw.setdefault('missing', _missing(c))
    out = E.run_cd_ekf_nll_grad(drift, disp.outer() if gamma is None else gamma, c['H'] if H is None else H, c['Xi'], m0_ if m0 is None else m0,
                                P0_ if P0 is None else P0, c['dt'], ys, dirs, **kw)
    return tuple(o.cpu().numpy() for o in out)


# ------------------------------------------------------------------------------------------------ 1. every fixture case
@pytest.mark.parametrize('name', NAMES)
def test_fixture_case(name):
    """Every case through the raw C-ABI (output buffers pre-filled) and through mle.value_and_grad (other_cd_H_dXi: through the engine
    call, which takes its H and the seventh direction d Xi = 1): the same bits from both, within the gates of the 100-digit numbers.  The
    gapped cases run with CGP_SKIP_MISSING / missing='skip'; the record of NaN only gives exactly 0 and a zero gradient."""
    c = case(name)
    dirs = directions(c)
    rc, msg, nll, grad = raw(c, c['ys'].size, dirs[0], FILL, flags=SKIP_MISSING if c['skip'] else 0)
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
    if name == 'gaps_cd_everywhere':
        assert nll[0] == 0.0 and not np.signbit(nll[0]) and np.array_equal(grad[0], np.zeros(6))


# ------------------------------------------------------------------------------------------------ 2. record lengths
@pytest.mark.parametrize('name', ['prefix_cd_chirp', 'prefix_cd_lascala'])
def test_record_lengths(name):
    """Measurements are fetched eight steps at a time with a zero-filled tail: T = 1, 2, 7, 8, 9, 64, 65, 130 against the 100-digit value
    and gradient of every prefix of one record, raw C-ABI and mle."""
    c = case(name)
    want_f, want_g = Z[f'{name}.nll_prefix'], Z[f'{name}.grad_prefix']
    dirs = directions(c)[0]
    worst = [0., 0.]
    for T in PREFIX_T:
        rc, msg, nll, grad = raw(c, T, dirs, FILL)
        assert rc == 0, msg
        f, g_ = _vg(c, T=T)
        npt.assert_array_equal(f, nll)
        npt.assert_array_equal(g_, grad)
        ev, eg = errors(nll[0], grad[0], want_f[T - 1], want_g[T - 1], f'{name} T = {T}')
        worst = [max(worst[0], ev), max(worst[1], eg)]
        assert ev < VALUE_RTOL and eg < GRAD_GATE, (T, nll[0], want_f[T - 1], grad[0], want_g[T - 1])
    print(f'{name}: worst over the record lengths: value {worst[0]:.2e}, gradient {worst[1]:.2e}')


def test_an_empty_record_writes_zeros():
    c = case('prefix_cd_chirp')
    rc, msg, nll, grad = raw(c, 0, directions(c)[0], np.nan)
    assert rc == 0, msg
    assert np.array_equal(nll, [0.0]) and np.array_equal(grad, np.zeros((1, 6)))
    f, g_ = _vg(c, ys=np.zeros(0))
    assert np.array_equal(f, [0.0]) and np.array_equal(g_, np.zeros((1, 6)))


# ------------------------------------------------------------------------------------------------ 3. the value is cd_ekf's
def test_the_value_is_cd_ekfs_final_nll():
    """On every fixture case the value equals the final NLL of filters_smoothers.cd_ekf on the same inputs to 1e-11 relative (the gapped
    cases with missing='skip' on both sides; the record of NaN only: both exactly 0)."""
    from chirpgp_amd import filters_smoothers as fs, models as pm
    worst = 0.0
    for name in NAMES:
        c = case(name)
        drift, disp, _, m0, P0, _ = builder(c['build'])(pm.g(c['theta']))
        want = float(np.asarray(fs.cd_ekf(drift, disp, c['H'], c['Xi'], m0, P0, c['dt'], c['ys'], nll_final_only=True, want=(False, False, True),
                                          missing=_missing(c))[2]).reshape(-1)[0])
        f, _ = _run_dirs(c, directions(c))
        err = abs(f[0] - want) / (abs(want) if want != 0 else 1.0)
        print(f'{name}: {f[0]!r} against cd_ekf {want!r}: {err:.2e}')
        worst = max(worst, err)
        assert err < VALUE_RTOL, name
    print(f'worst: {worst:.2e}')


# ------------------------------------------------------------------------------------------------ 4. launch shapes
def _chirp_thetas():
    rows = [Z['prefix_cd_chirp.theta']] + [Z[f'{n}.theta'] for n in NAMES if n.startswith('random_cd') and str(Z[f'{n}.build']) == 'chirp']
    return np.stack(rows)


def _dirs_n(c, thetas, n_dir):
    """n_dir directions per trial: the first four parameter directions, all six, or the six and d Xi = 1."""
    d = directions(c, thetas)
    if n_dir <= 6:
        return np.ascontiguousarray(d[:, :n_dir])
    d7 = np.zeros((thetas.shape[0], 1, 27))
    d7[:, 0, 12] = 1.0
    return np.concatenate([d, d7], axis=1)


@pytest.mark.parametrize('n_dir', [4, 6, 7])
def test_launch_shapes(n_dir):
    """B = 1 (a single trial), 11 (66 lanes at n_dir = 6: a partial second wavefront), 22 (132 lanes: a trial straddling two wavefronts),
    every trial with its own parameters and gamma (param_stride, gamma_stride) on one shared record (ys_repeat = B): every trial's row
    equals its single-trial launch bit for bit; trial 0 (the prefix case's parameters) within the gates."""
    c = case('prefix_cd_chirp')
    T = 65
    pool = _chirp_thetas()
    thetas = pool[np.arange(22) % pool.shape[0]]
    alone = [_run_dirs(c, _dirs_n(c, thetas[t:t + 1], n_dir), thetas=thetas[t:t + 1], T=T) for t in range(22)]
    for B in (1, 11, 22):
        f, grad = _run_dirs(c, _dirs_n(c, thetas[:B], n_dir), thetas=thetas[:B], T=T, trials_per_record=B)
        assert f.shape == (B,) and grad.shape == (B, n_dir)
        for t in range(B):
            npt.assert_array_equal(f[t], alone[t][0][0], err_msg=f'B = {B} trial {t}')
            npt.assert_array_equal(grad[t], alone[t][1][0], err_msg=f'B = {B} trial {t}')
        m = min(n_dir, 6)
        want_f, want_g = Z['prefix_cd_chirp.nll_prefix'][T - 1], Z['prefix_cd_chirp.grad_prefix'][T - 1]
        assert abs(f[0] - want_f) / abs(want_f) < VALUE_RTOL
        assert np.abs(grad[0, :m] - want_g[:m]).max() / np.abs(want_g).max() < GRAD_GATE


def test_shared_model_indexed_records_and_per_trial_operands():
    """One parameter vector and one gamma for every trial (param_stride = gamma_stride = 0) with per-trial H, m0 and P0; and through mle
    three records picked and permuted by record_index (ys_index) with two parameter vectors each (ys_repeat = 2): bit-identical to the
    same trials launched one by one."""
    c = case('prefix_cd_chirp')
    B, T = 5, 65
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
    # ---- records by index, two parameter vectors a record
    ys = c['ys']
    recs = np.stack([ys, ys[::-1].copy(), 0.7 * ys + 0.3 * rng.standard_normal(ys.size), 1.1 * ys])
    index = np.array([2, 0, 3, 0])
    thetas = _chirp_thetas()[:8]
    f, grad = _vg(c, thetas=thetas, ys=recs, record_index=index)
    assert f.shape == (8,) and grad.shape == (8, 6)
    for t in range(8):
        ft, gt = _vg(c, thetas=thetas[t:t + 1], ys=recs[index[t // 2]])
        npt.assert_array_equal(ft[0], f[t], err_msg=f'trial {t}')
        npt.assert_array_equal(gt[0], grad[t], err_msg=f'trial {t}')
    f0, g0 = _vg(c, thetas=thetas[:1], ys=recs[0])
    ev, eg = errors(f0[0], g0[0], c['nll'], c['grad'], 'record 0, the case itself')
    assert ev < VALUE_RTOL and eg < GRAD_GATE


# ------------------------------------------------------------------------------------------------ 5. a diverged trial
def test_a_diverged_trial_is_nan_and_alone():
    """A P0 that is not positive definite for one trial of three: NaN in that trial's value and in every entry of its gradient, the other
    two bit-identical to the clean launch; make_objective(exact=True) turns a diverged value into (inf, zeros)."""
    from chirpgp_amd import models as pm
    c = case('prefix_cd_chirp')
    dirs = np.repeat(directions(c), 3, axis=0)
    _, _, _, _, P0, _ = builder(c['build'])(pm.g(c['theta']))
    P0s = np.repeat(np.asarray(P0)[None], 3, axis=0)
    clean_f, clean_g = _run_dirs(c, dirs, T=40, P0=P0s, shared_model=True, trials_per_record=3)
    assert np.isfinite(clean_f).all() and np.isfinite(clean_g).all()
    P0s[1] = np.diag([1.0, -1.0, 1.0, 1.0])
    f, grad = _run_dirs(c, dirs, T=40, P0=P0s, shared_model=True, trials_per_record=3)
    assert np.isnan(f[1]) and np.isnan(grad[1]).all(), (f, grad)
    npt.assert_array_equal(f[[0, 2]], clean_f[[0, 2]])
    npt.assert_array_equal(grad[[0, 2]], clean_g[[0, 2]])
    rc, msg, nll, g_ = raw(c, 40, dirs[0], FILL, P0=P0s[1])
    assert rc == 0 and np.isnan(nll).all() and np.isnan(g_).all(), (rc, msg, nll, g_)


# ------------------------------------------------------------------------------------------------ 6. the argument table
def _model_d6(a):
    a['model'].d, a['model'].n_harm = 6, 2


# (what is wrong, the edit that makes it so, the code) -- the codes of tests/test_gpu_tangent_arguments.py for the arguments the entry shares
FAULTS = [('dirs = NULL', lambda a: a.update(dirs=None), E_ARG),
          ('nll = NULL', lambda a: a.update(nll=None), E_ARG),
          ('grad = NULL', lambda a: a.update(grad=None), E_ARG),
          ('ys = NULL', lambda a: a.update(ys=None), E_ARG),
          ('model = NULL', lambda a: a.update(model=None), E_ARG),
          ('model.params = NULL', lambda a: setattr(a['model'], 'params', None), E_ARG),
          ('init = NULL', lambda a: a.update(init=None), E_ARG),
          ('init.H = NULL', lambda a: setattr(a['init'], 'H', None), E_ARG),
          ('init.Xi = NULL', lambda a: setattr(a['init'], 'Xi', None), E_ARG),
          ('init.m0 = NULL', lambda a: setattr(a['init'], 'm0', None), E_ARG),
          ('init.P0 = NULL', lambda a: setattr(a['init'], 'P0', None), E_ARG),
          ('ys_repeat = 0', lambda a: a.update(ys_repeat=0), E_ARG),
          ('ys_stride = -1', lambda a: a.update(ys_stride=-1), E_ARG),
          ('param_stride = 1', lambda a: setattr(a['model'], 'param_stride', 1), E_ARG),
          ('a d = 6 model', _model_d6, E_UNSUPPORTED),
          ('an LCD model id', lambda a: setattr(a['model'], 'model_id', 1), E_UNSUPPORTED),
          ('gamma = NULL', lambda a: setattr(a['model'], 'gamma', None), E_UNSUPPORTED),
          ('a stray flag bit', lambda a: a.update(flags=SKIP_MISSING | 0x2), E_ARG),
          ('B = 0', lambda a: a.update(B=0), 0)]


def test_argument_checks():
    """B = 1, T = 8, n_dir = 6, output buffers pre-filled: one faulty argument at a time gives its code, a refusal names the entry point, a
    stray flag is named, and the outputs stay as they were.  Then the good calls: T = 9 and T = 0."""
    c = case('prefix_cd_chirp')
    dirs = directions(c)[0]
    assert dirs.shape == (6, 27)
    for label, edit, code in FAULTS:
        rc, msg, nll, grad = raw(c, 8, dirs, FILL, edit=edit)
        print(f'{ENTRY}, {label}: {rc} {msg.decode() if msg else ""}')
        assert rc == code, (label, rc, msg)
        assert code != E_UNSUPPORTED or ENTRY.encode() in msg, (label, msg)
        if label == 'a stray flag bit':
            assert ENTRY.encode() in msg and b'CGP_WAVE_PER_TRIAL' in msg and b'0x2' in msg, msg
        npt.assert_array_equal(nll, FILL, err_msg=label)
        npt.assert_array_equal(grad, FILL, err_msg=label)
    rc, msg, nll, grad = raw(c, 9, dirs, FILL)
    assert rc == 0, msg
    want_f, want_g = Z['prefix_cd_chirp.nll_prefix'][8], Z['prefix_cd_chirp.grad_prefix'][8]
    assert abs(nll[0] - want_f) / abs(want_f) < VALUE_RTOL and np.abs(grad[0] - want_g).max() / np.abs(want_g).max() < GRAD_GATE
    rc, msg, nll, grad = raw(c, 0, dirs, FILL)
    assert rc == 0, msg
    npt.assert_array_equal(nll, 0.0)
    npt.assert_array_equal(grad, 0.0)


def test_the_front_ends_that_stay_refused():
    """The Fisher form of this kernel is not built: value_grad_fisher, standard_errors and fit_scoring refuse 'cd_ekf' by name; exact=True
    with missing='skip' stays refused in fit and fit_many; the engine call refuses directions of 24 doubles."""
    from chirpgp_amd import mle, models as pm
    c = case('prefix_cd_chirp')
    args = (pm.build_chirp_model, c['theta'][None, :], c['ys'], c['Xi'], c['dt'])
    with pytest.raises(ValueError, match='tangent kernel'):
        mle.value_grad_fisher(*args, method='cd_ekf')
    with pytest.raises(ValueError, match='Fisher form'):
        mle.standard_errors(pm.build_chirp_model, c['theta'], c['ys'], c['Xi'], c['dt'], method='cd_ekf')
    with pytest.raises(ValueError, match='Fisher form'):
        mle.fit_scoring('cd_ekf', pm.build_chirp_model, pm.g(c['theta']), c['ys'], c['Xi'], c['dt'])
    with pytest.raises(ValueError, match='tangent kernels know no gaps'):
        mle.fit('cd_ekf', pm.build_chirp_model, pm.g(c['theta']), c['ys'], c['Xi'], c['dt'], missing='skip', exact=True)
    with pytest.raises(ValueError, match='tangent kernels know no gaps'):
        mle.fit_many('cd_ekf', pm.build_chirp_model, pm.g(c['theta']), c['ys'][None, :], c['Xi'], c['dt'], missing='skip', exact=True)
    with pytest.raises(ValueError, match='27'):
        _run_dirs(c, np.zeros((1, 6, 24)))


# ------------------------------------------------------------------------------------------------ 7. records with gaps
def test_a_gap_free_record_gives_the_same_bits_with_and_without_the_flag():
    c = case('prefix_cd_chirp')
    dirs = directions(c)[0]
    for T in (9, 130):
        rc0, _, nll0, grad0 = raw(c, T, dirs, FILL)
        rc1, _, nll1, grad1 = raw(c, T, dirs, FILL, flags=SKIP_MISSING)
        assert rc0 == 0 and rc1 == 0
        npt.assert_array_equal(nll0, nll1)
        npt.assert_array_equal(grad0, grad1)
    f0, g0 = _vg(c)
    f1, g1 = _vg(c, missing='skip')
    npt.assert_array_equal(f0, f1)
    npt.assert_array_equal(g0, g1)


def test_gaps_without_the_flag_propagate_and_with_it_touch_their_trial_only():
    """Without the flag a NaN measurement is what it is in the reference: NaN in value and gradient.  With it, one gapped record among
    three leaves the other two trials' bits alone."""
    c, clean = case('gaps_cd_run'), case('prefix_cd_chirp')
    f, g_ = _vg(c, missing=None)
    assert np.isnan(f).all() and np.isnan(g_).all()
    recs = np.stack([clean['ys'][:80], c['ys'], clean['ys'][:80][::-1].copy()])
    thetas = np.repeat(c['theta'][None, :], 3, axis=0)
    f, g_ = _vg(c, thetas=thetas, ys=recs, missing='skip')
    for t in (0, 2):
        ft, gt = _vg(clean, ys=recs[t])
        npt.assert_array_equal(ft[0], f[t])
        npt.assert_array_equal(gt[0], g_[t])
    ev, eg = errors(f[1], g_[1], c['nll'], c['grad'], 'the gapped record among three')
    assert ev < VALUE_RTOL and eg < GRAD_GATE


# ------------------------------------------------------------------------------------------------ 8. the L-BFGS front ends
def test_make_objective_and_fit_with_the_exact_gradient():
    """make_objective('cd_ekf', exact=True) returns value_and_grad's numbers; exact=None stays the difference route; fit(exact=True) on
    the T = 600 record of tests/test_gpu_mle_oracle.py ends within 1e-6 relative of the NLL the default difference-gradient fit reaches
    from the same start; fit_many(exact=True) takes the same route."""
    from chirpgp_amd import mle, models as pm
    from tests.test_gpu_mle_oracle import INIT, _record
    ys = _record(600, 556)
    theta = pm.g_inv(INIT)
    fun = mle.make_objective('cd_ekf', pm.build_chirp_model, ys, 0.1, 1e-3, exact=True)
    f, g_ = fun(theta)
    vf, vg = mle.value_and_grad(pm.build_chirp_model, theta[None, :], ys, 0.1, 1e-3, method='cd_ekf')
    assert f == vf[0] and np.array_equal(g_, vg[0])
    fd, gd = mle.make_objective('cd_ekf', pm.build_chirp_model, ys, 0.1, 1e-3)(theta)                  # exact=None: 13 probes
    assert abs(fd - f) <= 1e-11 * abs(f) and not np.array_equal(gd, g_)
    npt.assert_allclose(gd, g_, rtol=0, atol=2e-6 * np.abs(g_).max())
    opt, res = mle.fit('cd_ekf', pm.build_chirp_model, INIT, ys, 0.1, 1e-3, exact=True)
    opt_d, res_d = mle.fit('cd_ekf', pm.build_chirp_model, INIT, ys, 0.1, 1e-3)
    print(f'fit exact: nll {res.fun!r} in {res.nit} iterations ({res.nfev} launches); differences: {res_d.fun!r} in {res_d.nit} ({res_d.nfev}); '
          f'relative distance {abs(res.fun - res_d.fun) / abs(res_d.fun):.2e}')
    assert abs(res.fun - res_d.fun) <= 1e-6 * abs(res_d.fun), (res.fun, res_d.fun)
    start, _ = mle.value_and_grad(pm.build_chirp_model, theta[None, :], ys[:200], 0.1, 1e-3, method='cd_ekf')
    many, info = mle.fit_many('cd_ekf', pm.build_chirp_model, INIT, ys[None, :200], 0.1, 1e-3, maxiter=3, exact=True)
    assert np.isfinite(info['fun']).all() and info['fun'][0] < start[0] and info['nit'][0] >= 1
