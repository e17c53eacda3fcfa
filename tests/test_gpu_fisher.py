"""The Fisher information of the filters' Gaussian innovations model from the tangent kernels -- cgp_ekf_nll_fisher (csrc/cgp_tangent4.hpp,
kFisher) and cgp_sgp_nll_fisher (csrc/cgp_tangent4_sigma.hpp, kFisher):

    F[i][j] = sum_t ( d nu_i d nu_j / S + d S_i d S_j / (2 S^2) )

against 100-digit arithmetic (tests/golden/exact_fisher.npz, tests/golden/make_exact_fisher.py), and the layer on top of it in
chirpgp_amd/mle.py: value_grad_fisher, standard_errors, fit_scoring.

Measured on MI355X (gfx950), every case of the fixture (gate 1e-8 of the matrix's largest entry, the gradient's own):
  * cgp_ekf_nll_fisher, 14 cases: fisher <= 9.5e-13, value <= 3.3e-13, gradient <= 7.9e-13 of its scale (all three random_ekf_21);
  * cgp_sgp_nll_fisher, 8 cases: fisher <= 7.5e-11, value <= 6.8e-13, gradient <= 1.6e-9 of its scale (all three random_gh3_08);
  * directions D A against A^T F A: 1.5e-15 / 8.8e-15 of scale; value and gradient equal the gradient kernels' bit for bit on the three cases;
  * the perf test (CGP_RUN_PERF=1): cgp_ekf_nll_grad 3.298 ms, cgp_ekf_nll_fisher 3.892 ms, ratio 1.180 (1.260 in the 8-slot kernel);
  * every new test fails on the parent commit: the entry points do not exist there."""
import ctypes as C
import functools

import numpy as np
import numpy.testing as npt
import pytest

from tests.tangent_cases import ZF, builder as _builder, directions as _directions, fisher_case as _case, raw, run_dirs, sigma as _sigma

pytestmark = pytest.mark.gpu
NAMES = [str(n) for n in ZF['names']]
VALUE_RTOL, GRAD_GATE, FISHER_GATE = 1e-11, 1e-8, 1e-8
INIT = np.array([0.1, 0.1, 0.1, 1., 1., 7.])
_results = {}
_run_dirs = functools.partial(run_dirs, fisher=True)     # the raw engine call E.run_*_nll_fisher (fisher=False: run_*_nll_grad)


def _fixture_result(name):
    """(nll, grad, F) of a fixture case, computed once: mle.value_grad_fisher, or -- a measurement row other than the builder's and the
    direction whose only entry is dXi = 1, which mle does not take -- the raw engine call."""
    if name not in _results:
        from chirpgp_amd import mle
        c = _case(name)
        if c['with_dxi']:
            d7 = np.zeros((1, 1, 24))
            d7[0, 0, 9] = 1.0
            f, g, F = _run_dirs(c, np.concatenate([_directions(c), d7], axis=1), H=c['H'])
        else:
            f, g, F = mle.value_grad_fisher(_builder(c['build']), c['theta'][None, :], c['ys'], c['Xi'], c['dt'], method=c['method'],
                                            sgps=_sigma(c['sigma']))
        ev = abs(f[0] - c['nll']) / abs(c['nll'])
        eg = float(np.abs(g[0] - c['grad']).max() / np.abs(c['grad']).max())
        eF = float(np.abs(F[0] - c['fisher']).max() / np.abs(c['fisher']).max())
        _results[name] = (c, f, g, F, ev, eg, eF)
    return _results[name]


# ------------------------------------------------------------------------------------------------ 1., 2. every fixture case
@pytest.mark.parametrize('name', NAMES)
def test_fixture_case(name):
    """F within 1e-8 of its largest entry -- the project's gradient gate: the same tangents are multiplied -- with the value at rtol 1e-11
    and the gradient at 1e-8 of its scale against exact_grad_cases.npz; F exactly symmetric."""
    c, f, g, F, ev, eg, eF = _fixture_result(name)
    print(f'{name}: value error {ev:.2e}, gradient error {eg:.2e} of its scale, fisher error {eF:.2e} of its scale {np.abs(c["fisher"]).max():.3g}')
    assert F.shape == (1,) + c['fisher'].shape
    npt.assert_array_equal(F, F.transpose(0, 2, 1))
    assert eF < FISHER_GATE, (F[0], c['fisher'])
    assert ev < VALUE_RTOL, (f[0], c['nll'])
    assert eg < GRAD_GATE, (g[0], c['grad'])


def test_no_fixture_case_is_left_out_and_the_worst_per_method():
    """All 22 cases of the generator's list are in the file and run above; the worst errors per kernel, for README.md / DESIGN.md."""
    from tests.golden import make_exact_fisher as gen
    assert sorted(NAMES) == sorted(n for line in gen.CASES for n in line)
    for method in ('ekf', 'sgp_filter'):
        rows = [r for r in map(_fixture_result, NAMES) if r[0]['method'] == method]
        worst = {label: max(rows, key=lambda r: r[k]) for label, k in (('value', 4), ('gradient', 5), ('fisher', 6))}
        print(f'{method}, {len(rows)} cases: ' + ', '.join(f'worst {label} error {r[k]:.2e} ({r[0]["name"]})'
                                                           for (label, r), k in zip(worst.items(), (4, 5, 6))))
        assert rows


# ------------------------------------------------------------------------------------------------ 3. the lane mapping
def _mixed_batch(n_dir, n_trials, T, seed):
    """Distinct parameter vectors, directions (seeded combinations of the six tangent directions) and records for n_trials trials; trial t
    reads record t // 2."""
    from tests.test_gpu_gradient import _record
    rng = np.random.default_rng(seed)
    thetas = np.log(np.expm1(INIT * 2.0 ** rng.uniform(-0.5, 0.5, size=(n_trials, 6))))
    c = dict(build='chirp', method='ekf', sigma='', Xi=0.1, dt=1e-3)
    D = _directions(c, thetas)                                           # (n_trials, 6, 24)
    dirs = np.einsum('tik,tkc->tic', rng.standard_normal((n_trials, n_dir, 6)), D)
    recs = np.stack([_record(T, 900 + r) for r in range((n_trials + 1) // 2)])
    return thetas, dirs, recs


def _check_mapping(c, n_dir, B, seed):
    thetas, dirs, recs = _mixed_batch(n_dir, B + B % 2, 40, seed)
    alone = [_run_dirs(c, dirs[t:t + 1], thetas=thetas[t:t + 1], ys=recs[t // 2]) for t in range(B + B % 2)]
    want = [np.concatenate([a[k] for a in alone]) for k in range(3)]
    assert all(np.isfinite(w).all() for w in want) and want[2].shape == (B + B % 2, n_dir, n_dir)
    runs = {'own rows': (B, dict(ys=recs[np.arange(B) // 2])),
            'record_index': (B, dict(ys=recs, record_index=np.arange(B) // 2)),
            'trials_per_record = 2': (B + B % 2, dict(ys=recs, trials_per_record=2))}
    for label, (n, kw) in runs.items():
        got = _run_dirs(c, dirs[:n], thetas=thetas[:n], **kw)
        for k, what in enumerate(('nll', 'grad', 'fisher')):
            npt.assert_array_equal(got[k], want[k][:n], err_msg=f'{what}, n_dir {n_dir}, B {n}, {label}')


@pytest.mark.parametrize('n_dir,B', [(1, 65), (6, 11), (7, 10), (16, 5)])
def test_ekf_lane_mapping_is_the_trial_alone(n_dir, B):
    """64 / n_dir whole trials per wavefront: 64 trials and a second wavefront for one more (1, 65); ten trials of six lanes and four idle
    lanes, then one (6, 11); nine trials of seven lanes and ONE idle lane, then one (7, 10); four trials of sixteen lanes, then one
    (16, 5).  T = 40 (five 8-step blocks), distinct parameters, directions and records: every trial's nll, grad and F bit-identical to the
    same trial launched alone (B = 1), through each trial's own row, through record_index and with two trials per record (an odd B
    takes one trial more there)."""
    _check_mapping(dict(build='chirp', method='ekf', sigma='', Xi=0.1, dt=1e-3), n_dir, B, 100 * n_dir + B)


def test_sgp_lane_mapping_is_the_trial_alone():
    """One wavefront per trial, the owners' rows side by side in fisher[trial]: cubature, six directions, B = 3."""
    _check_mapping(dict(build='chirp', method='sgp_filter', sigma='cubature', Xi=0.1, dt=1e-3), 6, 3, 63)


# ------------------------------------------------------------------------------------------------ 4. linearity in the directions
@pytest.mark.parametrize('name', ['prefix_ekf', 'random_cubature_00'])
def test_fisher_is_a_quadratic_form_in_the_directions(name):
    """Directions D A (seeded random 6 x 6 A) give A^T F A within 1e-10 of its scale; the gradient gives A^T grad."""
    c = _case(name)
    D = _directions(c)[0]                                                # (6, 24)
    A = np.random.default_rng(2024).standard_normal((6, 6))
    f0, g0, F0 = _run_dirs(c, D[None])
    f1, g1, F1 = _run_dirs(c, (A.T @ D)[None])
    want = A.T @ F0[0] @ A
    err = np.abs(F1[0] - want).max() / np.abs(want).max()
    print(f'{name}: F(D A) against A^T F(D) A: {err:.2e} of its scale')
    assert err < 1e-10
    npt.assert_array_equal(f1, f0)
    npt.assert_allclose(g1[0], A.T @ g0[0], rtol=0, atol=1e-10 * np.abs(A.T @ g0[0]).max())


# ------------------------------------------------------------------------------------------------ 5. value and gradient are the gradient kernels'
@pytest.mark.parametrize('name', ['random_ekf_00', 'random_gh3_00', 'random_cubature_00'])
def test_value_and_gradient_are_the_gradient_kernels(name):
    """Within 1e-11 of scale of cgp_ekf_nll_grad / cgp_sgp_nll_grad (the same step body; the compiler may fuse it differently)."""
    c = _case(name)
    D = _directions(c)
    f0, g0 = _run_dirs(c, D, fisher=False)
    f1, g1, _ = _run_dirs(c, D)
    print(f'{name}: value differs by {abs(f1[0] - f0[0]) / abs(f0[0]):.2e}, gradient by {np.abs(g1 - g0).max() / np.abs(g0).max():.2e} of its scale')
    npt.assert_allclose(f1, f0, rtol=1e-11)
    npt.assert_allclose(g1, g0, rtol=0, atol=1e-11 * np.abs(g0).max())


# ------------------------------------------------------------------------------------------------ 6. edges
def _raw(entry, c, T, n_dir, B=1, fisher=True, fill=123.0, P0=None):
    """The C entry point itself with output buffers pre-filled with `fill`: -> (return code, message, nll, grad, fisher)."""
    return raw(entry, c, T, np.resize(_directions(c)[0], (n_dir, 24)), fill, B=B, P0=P0, edit=None if fisher else lambda a: a.update(fisher=None))


@pytest.mark.parametrize('entry', ['cgp_ekf_nll_fisher', 'cgp_sgp_nll_fisher'])
def test_argument_edges(entry):
    """T = 0 writes zeros to all three outputs; n_dir = 17 is refused (-2) with a message naming the limit; fisher = NULL is -1; B = 0
    returns 0 and writes nothing."""
    c = _case('prefix_ekf' if entry == 'cgp_ekf_nll_fisher' else 'random_cubature_00')
    rc, msg, nll, grad, F = _raw(entry, c, 0, 6)
    assert rc == 0, msg
    npt.assert_array_equal(nll, 0.0); npt.assert_array_equal(grad, 0.0); npt.assert_array_equal(F, 0.0)
    rc, msg, nll, grad, F = _raw(entry, c, 8, 17)
    assert rc == -2 and b'CGP_FISHER_MAX_DIR' in msg and b'16' in msg, (rc, msg)
    npt.assert_array_equal(F, 123.0)
    rc, msg, nll, grad, F = _raw(entry, c, 8, 6, fisher=False)
    assert rc == -1 and b'fisher' in msg, (rc, msg)
    npt.assert_array_equal(grad, 123.0)
    rc, msg, nll, grad, F = _raw(entry, c, 8, 6, B=0)
    assert rc == 0, msg
    npt.assert_array_equal(nll, 123.0); npt.assert_array_equal(F, 123.0)
    rc, msg, nll, grad, F = _raw(entry, c, 8, 16)                         # the limit itself runs
    assert rc == 0 and np.isfinite(F).all(), (rc, msg)
    npt.assert_array_equal(F, F.transpose(0, 2, 1))


def test_a_cholesky_that_breaks_down_writes_nan_to_all_three():
    """A P0 that is not positive definite, through the raw call: the sigma-point filter's factorisation fails at the first step; nll,
    grad and every entry of F are NaN (as sgp_filter writes NaN), not stale buffer contents and not a fault."""
    c = _case('random_cubature_00')
    P0 = np.diag([1.0, -1.0, 1.0, 1.0])
    rc, msg, nll, grad, F = _raw('cgp_sgp_nll_fisher', c, 20, 6, P0=P0)
    assert rc == 0, msg
    assert np.isnan(nll).all() and np.isnan(grad).all() and np.isnan(F).all(), (nll, grad, F)


def test_more_than_sixteen_directions_through_the_engine_is_an_error():
    """No quiet slicing: the matrix couples all the directions of a launch."""
    c = _case('prefix_ekf_T8')
    dirs = np.resize(_directions(c)[0], (1, 17, 24))
    with pytest.raises(RuntimeError, match='CGP_FISHER_MAX_DIR'):
        _run_dirs(c, dirs)
    from chirpgp_amd import mle, models as pm
    with pytest.raises(ValueError, match='tangent kernel'):
        mle.value_grad_fisher(pm.build_chirp_model, c['theta'][None, :], c['ys'], c['Xi'], c['dt'], method='cd_ekf')


# ------------------------------------------------------------------------------------------------ 7. standard errors at an optimum
def test_standard_errors_at_the_optimum_of_the_demos_record():
    """The T = 3141 record of test_fit_with_exact_gradients at its optimum: finite positive standard errors, or the singular flag.  F is
    printed beside the central-difference Hessian of the exact gradient -- recorded, not gated: the two differ by terms of zero mean
    (nu d^2 nu / S and the like), which one record does not average away."""
    from chirpgp_amd import mle, models as pm
    from tests.test_gpu_gradient import _record
    ys = _record(3141, 555)
    opt, res = mle.fit('ekf', pm.build_chirp_model, INIT, ys, 0.1, 1e-3, maxiter=300, exact=True)
    se, cov, info = mle.standard_errors(pm.build_chirp_model, res.x, ys, 0.1, 1e-3)
    with np.printoptions(precision=4, linewidth=200):
        print(f'nll {info["nll"]:.9g}, cond of the scaled information {info["cond"]:.3g}, singular {info["singular"]}')
        print('parameters     ', opt)
        print('standard errors', se)
        npt.assert_allclose(info['nll'], res.fun, rtol=1e-11)
        npt.assert_array_equal(info['fisher'], info['fisher'].T)
        if info['singular']:
            assert np.all(np.isinf(se)) and np.all(np.isinf(cov))
        else:
            assert np.all(np.isfinite(se)) and np.all(se > 0)
            npt.assert_allclose(cov @ info['fisher'], np.eye(6), atol=1e-6)
        h = 1e-4 * (1.0 + np.abs(res.x))
        probes = np.concatenate([res.x + np.diag(h), res.x - np.diag(h)])
        _, gp = mle.value_and_grad(pm.build_chirp_model, probes, ys, 0.1, 1e-3)
        hess = (gp[:6] - gp[6:]) / (2 * h[:, None])
        hess = 0.5 * (hess + hess.T)
        print('Fisher information F (unconstrained theta):\n', info['fisher'])
        print('central-difference Hessian of the exact gradient:\n', hess)
        d = np.sqrt(np.diag(info['fisher']))
        print('(hessian - F) / sqrt(F_ii F_jj):\n', (hess - info['fisher']) / np.outer(d, d))


# ------------------------------------------------------------------------------------------------ 8. Fisher scoring
def test_fit_scoring_in_lock_step():
    """The three T = 1200 records of test_lockstep_fit_many_takes_the_tangent_kernel: every record ends by the gradient rule within
    maxiter, and no accepted step increases the NLL.  Launches and final NLL are printed beside fit_many(exact=True)'s; equality of the
    optima is not asserted (the two may stop in different basins)."""
    from chirpgp_amd import mle, models as pm
    from tests.test_gpu_gradient import _record
    recs = np.stack([_record(1200, 700 + r) for r in range(3)])
    opt, info = mle.fit_scoring('ekf', pm.build_chirp_model, INIT, recs, 0.1, 1e-3, maxiter=100)
    many, info_l = mle.fit_many('ekf', pm.build_chirp_model, INIT, recs, 0.1, 1e-3, maxiter=200, exact=True)
    print(f'scoring: {info["launches"]} launches, iterations {info["nit"]}, nll {info["fun"]}, max |grad| {np.abs(info["grad"]).max(axis=1)}')
    print(f'L-BFGS (fit_many, exact): {info_l["launches"]} launches, iterations {info_l["nit"]}, nll {info_l["fun"]}')
    print('scoring parameters\n', opt, '\nL-BFGS parameters\n', many)
    assert info['converged'].all(), (info['converged'], info['mu'])
    assert np.all(np.abs(info['grad']).max(axis=1) <= 1e-5 * np.maximum(1.0, np.abs(info['fun'])))
    hist, path = np.array(info['history']), np.array(info['iterates'])   # every record's NLL and iterate after every launch
    n = info['launches']
    assert hist.shape == (n, 3) and path.shape == (n, 3, 6) and n <= 101
    assert info['fisher'].shape == (3, 6, 6) and np.isfinite(info['fisher']).all()
    # history only ever takes a smaller value, so its own differences show nothing: the NLL is evaluated AGAIN, in one launch, at the
    # iterates the fit held after seven of its launches (first, second, quartiles, last), and those values must be the recorded ones and
    # must not increase from one to the next -- an accepted step that did not lower the NLL at the iterate it stored fails here
    at = np.unique([0, 1, n // 4, n // 2, 3 * n // 4, n - 2, n - 1])
    again, _, _ = mle.value_grad_fisher(pm.build_chirp_model, path[at].reshape(-1, 6), recs, 0.1, 1e-3, record_index=np.tile(np.arange(3), at.size))
    again = again.reshape(at.size, 3)
    print('launch', at, '\nNLL evaluated again at the stored iterates\n', again)
    npt.assert_allclose(again, hist[at], rtol=1e-9)
    assert np.all(np.diff(again, axis=0) <= 0) and np.all(again[-1] < again[0])
    npt.assert_array_equal(pm.g(path[-1]), opt)
    npt.assert_array_equal(hist[-1], info['fun'])


# ------------------------------------------------------------------------------------------------ timing
@pytest.mark.perf
def test_the_fisher_launch_costs_a_quarter_more_at_most():
    """cgp_ekf_nll_fisher against cgp_ekf_nll_grad in one process: 1500 records x T = 3141, 6 directions, the median of 20 launches after
    warm-up.  Bound 1.25, set when the addition was counted as about 45 vector instructions on about 520 a step, off the recurrence's
    dependence chain, with margin for the idle lanes of the whole-trial mapping.  The disassembly has 72 more on 570 at six directions
    (6-slot kernel: 28 of vector arithmetic, 24 shuffles, 12 moves to and from AGPRs, 11 waits); the bound stays.
    (A timing assertion: CGP_RUN_PERF=1 only.)"""
    import torch
    from chirpgp_amd import _engine as E, models as pm
    from tests.test_gpu_gradient import _record
    R, T = 1500, 3141
    ys = E.dev(_record(T, 555)[None, :] + 0.05 * np.random.default_rng(1).standard_normal((R, T)))
    thetas = np.tile(pm.g_inv(INIT), (R, 1))
    dirs = E.dev(_directions(dict(build='chirp', dt=1e-3, Xi=0.1), thetas))
    drift, disp, disc, m0, P0, H = pm.build_chirp_model(pm.g(thetas))
    lib, ctx, keep = E.load_library(), E.context(), []
    model, init = E._model_struct(disc, None, R, keep), E._init_struct(H, 0.1, m0, P0, 4, R, keep)
    opts = dict(dtype=torch.float64, device='cuda')
    nll, grad, F = torch.empty((R,), **opts), torch.empty((R, 6), **opts), torch.empty((R, 6, 6), **opts)
    head = (ctx, C.byref(model), C.byref(init), 1e-3, ys.data_ptr(), T, 1, None, R, T, dirs.data_ptr(), 6, nll.data_ptr(), grad.data_ptr())
    launch = {'grad': lambda: lib.cgp_ekf_nll_grad(*head, 0, E._stream()), 'fisher': lambda: lib.cgp_ekf_nll_fisher(*head, F.data_ptr(), 0, E._stream())}
    med = {}
    for name in ('grad', 'fisher', 'grad', 'fisher'):                    # (twice each, interleaved: the later median of a kernel stands)
        times = []
        for i in range(23):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            assert launch[name]() == 0
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_time(stop))
        med[name] = float(np.median(times[3:]))
    ratio = med['fisher'] / med['grad']
    print(f'cgp_ekf_nll_grad {med["grad"]:.3f} ms, cgp_ekf_nll_fisher {med["fisher"]:.3f} ms: ratio {ratio:.3f}')
    assert ratio <= 1.25, ratio
