"""The sigma-point filter's MLE objective with its EXACT gradient (cgp_sgp_nll_grad): forward tangents of (m, P, nll) through the scan
of sgp_filter -- the Cholesky factor's tangent, every sigma point's, the predicted moments' and the update's -- where the reference takes
jax.value_and_grad through the scan (demos/ghfs_mle.py:53-56).  Checked against the derivative computed in 100-digit arithmetic
(tests/golden/exact_sgp_grad.npz), against the engine's own sgp_filter, against the oracle's fourth-order difference quotient at the
demos' record length, and through the optimisers."""
import ctypes as C
import os

import numpy as np
import numpy.testing as npt
import pytest

from tests import mle_oracle as mo

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'exact_sgp_grad.npz')
INIT = np.array([0.1, 0.1, 0.1, 1., 1., 7.])
LASCALA_INIT = np.array([0.1, 1., 1., 7.])


def _record(T, seed, dt=1e-3, Xi=0.1):
    from chirpgp_amd.toymodels import gen_chirp, meow_freq, constant_mag
    ts = np.linspace(dt, dt * T, T)
    _, phase = meow_freq(offset=8.)
    return gen_chirp(ts, constant_mag(1.), phase) + np.sqrt(Xi) * np.random.default_rng(seed).standard_normal(T)


def _gh3():
    from chirpgp_amd.quadratures import SigmaPoints
    return SigmaPoints.gauss_hermite(4, 3)


def _sigma(name):
    from chirpgp_amd.quadratures import SigmaPoints
    return SigmaPoints.gauss_hermite(4, 3) if name == 'gh3' else SigmaPoints.cubature(4)


def _builder(name):
    from chirpgp_amd import models as pm
    return pm.build_chirp_model if name == 'chirp' else pm.build_lascala_model


@pytest.mark.parametrize('name', ['gh3_track', 'gh3_lost', 'cubature_track', 'lascala_gh3_track'])
def test_value_and_gradient_against_100_digit_arithmetic(name):
    """Value 1e-11, gradient 1e-8 of its scale (the EKF tangent kernel's gates); the 13-pass difference form's error printed beside."""
    from chirpgp_amd import mle
    z = np.load(GOLD)
    theta, ys, Xi, dt = z[f'{name}.theta'], z[f'{name}.ys'], float(z[f'{name}.Xi']), float(z[f'{name}.dt'])
    build, sg = _builder(str(z[f'{name}.build'])), _sigma(str(z[f'{name}.sigma']))
    f, grad = mle.value_and_grad(build, theta[None, :], ys, Xi, dt, method='sgp_filter', sgps=sg)
    want = z[f'{name}.grad']
    err = np.abs(grad[0] - want).max() / np.abs(want).max()
    fun = mle.make_objective('sgp_filter', build, ys, Xi, dt, sgps=sg, exact=False)
    _, gfd = fun(theta)
    print(f'{name}: nll {f[0]:.12g} (exact {float(z[name + ".nll"]):.12g}), gradient error {err:.2e} of its scale {np.abs(want).max():.3g}; '
          f'central differences of {2 * theta.size + 1} passes: {np.abs(gfd - want).max() / np.abs(want).max():.2e}')
    npt.assert_allclose(f[0], float(z[f'{name}.nll']), rtol=1e-11)
    assert err < 1e-8, (grad, want)


def test_same_primal_as_sgp_filter():
    """The value is the engine's own sgp_filter(..., nll_final_only=True) on the same parameters, GH-3 and cubature: its literal sums over
    the points (LITERAL_SIGMA_SUM) and its default route (the collapsed quadrature on the matrix cores: an exact regrouping of the sums)."""
    from chirpgp_amd import _engine as E, filters_smoothers as fs, mle, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    ys = _record(1000, 11)
    th = np.stack([mo.g_inv(INIT), mo.g_inv(INIT * np.array([1.3, 2.0, 0.7, 1.5, 3.0, 1.2]))])
    drift, disp, disc, m0, P0, H = pm.build_chirp_model(pm.g(th))
    for sg in (SigmaPoints.gauss_hermite(4, 3), SigmaPoints.cubature(4)):
        f, _ = mle.value_and_grad(pm.build_chirp_model, th, ys, 0.1, 1e-3, method='sgp_filter', sgps=sg)
        kw = dict(nll_final_only=True, want=(False, False, True), trials_per_record=2)
        literal = np.asarray(fs.sgp_filter(disc, sg, H, 0.1, m0, P0, 1e-3, ys, flags=E.LITERAL_SIGMA_SUM, **kw)[2])
        default = np.asarray(fs.sgp_filter(disc, sg, H, 0.1, m0, P0, 1e-3, ys, **kw)[2])
        print(f'{sg.n_points} points: relative difference {np.abs(f / literal - 1).max():.2e} (literal sums), {np.abs(f / default - 1).max():.2e} (default route)')
        npt.assert_allclose(f, literal, rtol=2e-12)
        npt.assert_allclose(f, default, rtol=1e-11)                 # (4.96e-12 at 81 points: rounding of the regrouped sums, amplified)


def test_gradient_at_the_demos_record_length_and_batched():
    """T = 3141 (demos/ghfs_mle.py) against the oracle's fourth-order difference quotient; two parameter vectors per record on three
    records in ONE launch; a record_index subset bit-identical to the full launch's rows; the La Scala builder (4 parameters)."""
    from chirpgp_amd import mle, models as pm
    sg = _gh3()
    ys = _record(3141, 555)
    th = np.stack([mo.g_inv(INIT), mo.g_inv(INIT * np.array([1.3, 2.0, 0.7, 1.5, 3.0, 1.2]))])
    f, grad = mle.value_and_grad(pm.build_chirp_model, th, ys, 0.1, 1e-3, method='sgp_filter', sgps=sg)
    for i in range(2):
        f_o, g_o = mo.value_and_grad('sgp_filter', pm.build_chirp_model, th[i], ys, 0.1, 1e-3, sgps=sg)
        npt.assert_allclose(f[i], f_o, rtol=1e-9)
        npt.assert_allclose(grad[i], g_o, rtol=2e-7, atol=2e-7 * np.abs(g_o).max())
    recs = np.stack([_record(800, 600 + r) for r in range(3)])
    thetas = np.concatenate([th, th[::-1], th])                       # two parameter vectors per record, record-major
    f, grad = mle.value_and_grad(pm.build_chirp_model, thetas, recs, 0.1, 1e-3, method='sgp_filter', sgps=sg)
    for r in range(3):
        for j in range(2):
            f_o, g_o = mo.value_and_grad('sgp_filter', pm.build_chirp_model, thetas[2 * r + j], recs[r], 0.1, 1e-3, sgps=sg)
            npt.assert_allclose(f[2 * r + j], f_o, rtol=1e-9)
            npt.assert_allclose(grad[2 * r + j], g_o, rtol=2e-7, atol=2e-7 * np.abs(g_o).max())
    f1, g1 = mle.value_and_grad(pm.build_chirp_model, thetas[[2, 3]], recs, 0.1, 1e-3, record_index=[1], method='sgp_filter', sgps=sg)
    npt.assert_array_equal(f1, f[[2, 3]])
    npt.assert_array_equal(g1, grad[[2, 3]])
    la = mo.g_inv(LASCALA_INIT)
    f, grad = mle.value_and_grad(pm.build_lascala_model, la[None, :], recs[0], 0.1, 1e-3, method='sgp_filter', sgps=sg)
    f_o, g_o = mo.value_and_grad('sgp_filter', pm.build_lascala_model, la, recs[0], 0.1, 1e-3, sgps=sg)
    npt.assert_allclose(f[0], f_o, rtol=1e-9)
    npt.assert_allclose(grad[0], g_o, rtol=2e-7, atol=2e-7 * np.abs(g_o).max())


def test_breakdown_gives_nan_and_an_empty_record_gives_zeros():
    from chirpgp_amd import mle, models as pm
    sg = _gh3()
    ys = _record(300, 5)
    bad = mo.g_inv(INIT)
    bad[1] = 1e7                                                      # b = 1e7: the covariance stops being positive definite
    assert np.isnan(mo.nll('sgp_filter', pm.build_chirp_model, bad[None, :], ys, 0.1, 1e-3, sgps=sg)[0])
    f, grad = mle.value_and_grad(pm.build_chirp_model, np.stack([bad, mo.g_inv(INIT)]), ys, 0.1, 1e-3, method='sgp_filter', sgps=sg)
    assert np.isnan(f[0]) and np.isnan(grad[0]).all()
    assert np.isfinite(f[1]) and np.isfinite(grad[1]).all()          # a broken trial does not reach its neighbour
    fun = mle.make_objective('sgp_filter', pm.build_chirp_model, ys, 0.1, 1e-3, sgps=sg, exact=True)
    v, g_ = fun(bad)
    assert v == np.inf and np.array_equal(g_, np.zeros(6))
    f, grad = mle.value_and_grad(pm.build_chirp_model, mo.g_inv(INIT)[None, :], np.zeros(0), 0.1, 1e-3, method='sgp_filter', sgps=sg)
    assert np.array_equal(f, [0.0]) and np.array_equal(grad, np.zeros((1, 6)))


def test_fit_with_exact_gradients():
    """mle.fit on the tangent kernel reaches the oracle optimum (SciPy L-BFGS-B on the port's objective) on the demo's record."""
    from chirpgp_amd import mle, models as pm
    sg = _gh3()
    ys = _record(3141, 555)
    opt, res = mle.fit('sgp_filter', pm.build_chirp_model, INIT, ys, 0.1, 1e-3, sgps=sg, maxiter=300, exact=True)
    opt_o, res_o = mo.fit('sgp_filter', pm.build_chirp_model, INIT, ys, 0.1, 1e-3, sgps=sg)
    print(f'exact: nll {res.fun:.9g} in {res.nit} iterations ({res.nfev} launches); oracle + SciPy: {res_o.fun:.9g} in {res_o.nit} ({res_o.nfev})')
    npt.assert_allclose(res.fun, res_o.fun, rtol=1e-6)
    keep = np.array([2, 3, 4, 5])
    npt.assert_allclose(opt[keep], opt_o[keep], rtol=3e-3)
    assert opt[0] < 1e-6 and opt_o[0] < 1e-6                         # this optimum has no damping: lam sits at its boundary, 0
    npt.assert_allclose(mo.nll('sgp_filter', pm.build_chirp_model, pm.g_inv(opt), ys, 0.1, 1e-3, sgps=sg)[0], res.fun, rtol=1e-9)


def test_lockstep_fit_many_takes_the_tangent_kernel():
    from chirpgp_amd import mle, models as pm
    sg = _gh3()
    T, R = 1200, 3
    recs = np.stack([_record(T, 700 + r) for r in range(R)])
    many, info = mle.fit_many('sgp_filter', pm.build_chirp_model, INIT, recs, 0.1, 1e-3, sgps=sg, maxiter=200, exact=True)
    for r in range(R):
        _, res_o = mo.fit('sgp_filter', pm.build_chirp_model, INIT, recs[r], 0.1, 1e-3, sgps=sg)
        assert info['fun'][r] <= res_o.fun + 1e-5 * abs(res_o.fun), (r, info['fun'][r], res_o.fun)
    print('launches', info['launches'], 'fun', info['fun'])


def test_c_abi_argument_errors():
    import torch
    from chirpgp_amd import _engine as E, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    lib, ctx = E.load_library(), E.context()
    keep = []
    x = torch.zeros(64, dtype=torch.float64, device='cuda')
    p = x.data_ptr()
    sg4 = E._sigma_struct(SigmaPoints.gauss_hermite(4, 3), 4, keep)
    sg6 = E._sigma_struct(SigmaPoints.cubature(6), 6, keep)
    drift, disp, disc, m0, P0, H = pm.build_harmonic_chirp_model(INIT, 2)
    model6 = E._model_struct(disc, None, 1, keep)
    init6 = E._init_struct(H, 0.1, m0, P0, 6, 1, keep)
    rc = lib.cgp_sgp_nll_grad(ctx, C.byref(model6), C.byref(sg6), C.byref(init6), 1e-3, p, 64, 1, None, 1, 64, p, 1, p, p, 0, None)
    assert rc == -2 and b'd = 4' in lib.cgp_last_error(ctx)
    drift, disp, disc, m0, P0, H = pm.build_chirp_model(INIT)
    model = E._model_struct(disc, None, 1, keep)
    init = E._init_struct(H, 0.1, m0, P0, 4, 1, keep)
    rc = lib.cgp_sgp_nll_grad(ctx, C.byref(model), C.byref(sg6), C.byref(init), 1e-3, p, 64, 1, None, 1, 64, p, 1, p, p, 0, None)
    assert rc == -2 and b'd = 4' in lib.cgp_last_error(ctx)
    assert lib.cgp_sgp_nll_grad(ctx, C.byref(model), C.byref(sg4), C.byref(init), 1e-3, p, 64, 1, None, 1, 64, None, 1, p, p, 0, None) == -1
    assert lib.cgp_sgp_nll_grad(ctx, C.byref(model), C.byref(sg4), C.byref(init), 1e-3, p, 64, 0, None, 1, 64, p, 1, p, p, 0, None) == -1
    assert lib.cgp_sgp_nll_grad(ctx, C.byref(model), None, C.byref(init), 1e-3, p, 64, 1, None, 1, 64, p, 1, p, p, 0, None) == -1
    assert lib.cgp_sgp_nll_grad(ctx, C.byref(model), C.byref(sg4), C.byref(init), 1e-3, p, 64, 1, None, 0, 64, p, 1, p, p, 0, None) == 0
