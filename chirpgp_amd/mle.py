"""Maximum-likelihood parameter estimation through the filters -- the step every driver of the reference runs before
filtering and smoothing (demos/ekfs_mle.py:39-51, tetralith/jobs/*_mle.py).

The reference minimises ``obj(theta) = filter(build_model(g(theta)), ys)[-1][-1]`` with jaxopt's L-BFGS-B wrapper and
reverse-mode autodiff THROUGH the scan.  A HIP kernel is not JAX-differentiable; instead the engine's strengths are
used: the filters take one parameter vector per trial and an NLL-only output mode, so the objective and its central
finite-difference gradient -- 2 P + 1 filter passes over the same measurements -- are ONE kernel launch with a batch of
2 P + 1 "trials" (13 for the chirp model's 6 parameters) that all read the ONE copy of the record in HBM.  The optimiser itself stays SciPy's L-BFGS-B on the host,
exactly the algorithm the reference uses.
"""
import numpy as np

from chirpgp_amd import filters_smoothers as fs
from chirpgp_amd import models as M

__all__ = ['batched_nll', 'make_objective', 'fit', 'fit_many', 'grid_search', 'value_and_grad', 'tangent_directions', 'tangent_directions_cd', 'has_exact_gradient', 'has_tangent_kernel',
           'value_grad_fisher', 'covariance_from_fisher', 'standard_errors', 'scoring_step', 'fit_scoring']


def _rows_per_record(G, ys, record_index):
    """G parameter vectors shared out evenly over the records of ys -- (T,) or (R, T) -- or over the record_index entries: rows each."""
    n_rec = int(np.size(record_index)) if record_index is not None else 1 if np.ndim(ys) == 1 else int(np.shape(ys)[0])
    if n_rec < 1 or G % n_rec:
        raise ValueError(f'{G} parameter vectors cannot be shared out evenly over {n_rec} records')
    return G // n_rec


def _substeps_kw(method, substeps):
    """``substeps`` of an objective -> the filters' keyword.  1 .. 16, and more than one for 'cd_ekf' and 'cd_sgp_filter' only: checked here,
    before anything is built or launched."""
    from chirpgp_amd import _engine as E
    if not E.rk4_substeps(substeps):
        return {}
    if method not in ('cd_ekf', 'cd_sgp_filter'):
        raise ValueError(f"substeps goes with method 'cd_ekf' and 'cd_sgp_filter' only, not with {method!r}: a discrete model has no ODE to integrate")
    return dict(substeps=int(substeps))


def _exact_with_substeps(exact, method, substeps):
    """``exact`` of an objective with RK4 substeps: unchanged -- the tangent kernels of cd_ekf and cd_sgp_filter take the substeps.  The
    count and the method are checked here, before anything is built."""
    _substeps_kw(method, substeps)
    return exact


def _dts_kw(method, dts, dt, check=True):
    """``dts=`` of an objective (one interval per step in place of dt: filters_smoothers) -> the filters' keyword.  For 'cd_ekf' and
    'cd_sgp_filter' only, and dt must then be None: checked here, before anything is built or launched."""
    if dts is None:
        return {}
    if method not in ('cd_ekf', 'cd_sgp_filter'):
        raise ValueError(f"dts= goes with method 'cd_ekf' and 'cd_sgp_filter' only, not with {method!r}: a discrete model's constants are fixed per dt")
    if dt is not None:
        raise ValueError('pass either dt or dts=, not both: with dts= every step has its own interval and dt must be None')
    return dict(dts=dts, check_dts=check)


def _exact_with_times(exact, method, dts, dt):
    """``exact`` of an objective on a record with its own time stamps: the tangent kernels take one dt, so None resolves to the difference
    gradient and True is refused."""
    if dts is None:
        return exact
    _dts_kw(method, dts, dt)
    if exact:
        raise ValueError('exact=True does not go with dts=: the tangent kernels take one dt; the difference gradient (exact=False) takes the intervals')
    return False


def batched_nll(method, build, thetas, ys, Xi, dt, sgps=None, record_index=None, *, missing=None, substeps=1, dts=None, check_dts=True, **build_kw):
    """Final cumulative NLL of ``method`` for every row of ``thetas`` (unconstrained parameters, g() maps them to the
    positive model parameters as in the reference).  ``ys`` is ONE record (T,) read by all G rows, or R records (R, T) of
    which each serves G / R consecutive rows (``record_index`` (n,) first picks n of them: G / n rows each).  The records
    are read in place through the C-ABI's shared-record addressing (include/chirpgp_hip.h, cgp_filter): nothing is
    replicated, on the host or on the device.

    method: 'ekf' | 'sgp_filter' | 'cd_ekf' | 'cd_sgp_filter' with a 6-tuple builder (models.build_chirp_model,
    build_harmonic_chirp_model, build_lascala_model), or 'ekf_for_kpt' with models.build_kpt_chirp_model (pass ``fs=``,
    ``num_harmonics=``): tetralith/jobs/kpt_mle.py:41-44.

    ``missing='skip'``: NaN samples of the records are gaps (filters_smoothers: the likelihood of the observed samples alone).
    ``substeps=n`` ('cd_ekf', 'cd_sgp_filter'): n RK4 steps of dt / n between two measurements (filters_smoothers).
    ``dts=`` ('cd_ekf', 'cd_sgp_filter'; dt is then None): one interval per step, (T,) for all records or (R, T) one time grid per record
    of ys -- every row of a record reads the one copy of its grid, like its samples; ``check_dts=False``: the caller has checked the entries."""
    thetas = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    kw = dict(nll_final_only=True, want=(False, False, True), trials_per_record=_rows_per_record(thetas.shape[0], ys, record_index),
              record_index=record_index, missing=missing, **_substeps_kw(method, substeps), **_dts_kw(method, dts, dt, check_dts))
    with np.errstate(all='ignore'):        # a probe whose parameters under- or overflow yields a NaN objective, which the line search rejects
        built = build(M.g(thetas), **build_kw)
    if method == 'ekf_for_kpt':
        F, Sigma, m0, P0, h = built
        out = fs.ekf_for_kpt(F, Sigma, h, Xi, m0, P0, dt, ys, **kw)
    else:
        drift, disp, disc, m0, P0, H = built
        if method == 'ekf':
            out = fs.ekf(disc, H, Xi, m0, P0, dt, ys, **kw)
        elif method == 'sgp_filter':
            out = fs.sgp_filter(disc, sgps, H, Xi, m0, P0, dt, ys, **kw)
        elif method == 'cd_ekf':
            out = fs.cd_ekf(drift, disp, H, Xi, m0, P0, dt, ys, **kw)
        elif method == 'cd_sgp_filter':
            out = fs.cd_sgp_filter(drift, disp, sgps, H, Xi, m0, P0, dt, ys, **kw)
        else:
            raise ValueError(method)
    nll = out[2]
    return nll.cpu().numpy() if type(nll).__module__.startswith('torch') else np.asarray(nll)


# ---- exact gradients: forward tangents through the scan (include/chirpgp_hip.h: cgp_ekf_nll_grad, cgp_sgp_nll_grad) ------------
def _horner(x, coeffs):
    """sum_k coeffs[k] x^k (complex-safe)."""
    acc = coeffs[-1] + 0. * x
    for c in coeffs[-2::-1]:
        acc = acc * x + c
    return acc


_FACT = np.cumprod(np.r_[1., np.arange(1., 40.)])                       # k!
_SERIES_TERMS = 26                                                      # x <= 1: x^26 / 26! = 2.5e-27
_PHI = [(-1.) ** k / _FACT[k + 1] for k in range(_SERIES_TERMS)]         # (1 - exp(-x)) / x = sum (-x)^k / (k + 1)!
_PSI = [1. / _FACT[k + 3] for k in range(_SERIES_TERMS)]                 # (exp(x) - 1 - x - x^2 / 2) / x^3 = sum x^k / (k + 3)!
_F00 = [(-1.) ** k * (-1. - k) / _FACT[k + 2] for k in range(_SERIES_TERMS)]   # ((1 + x) exp(-x) - 1) / x^2 = sum (-1)^k (-1 - k) / (k + 2)! x^k


def _below(x, at, series, closed):
    """series where Re x < at, closed elsewhere (both complex-safe; the unused side may be NaN)."""
    return np.where(np.real(x) < at, series, closed)


def _decay_ratio(x):
    """(1 - exp(-x)) / x without the cancellation of its numerator -- nor of its DERIVATIVE's (x exp(-x) - (1 - exp(-x))) / x^2, which the
    complex step through expm1(-x) / x still carries at eps / x: the alternating series below x = 0.5 (x = 0 included), -expm1(-x) / x above."""
    safe = np.where(np.real(x) < 0.5, 1., x)
    return _below(x, 0.5, _horner(x, _PHI), -np.expm1(-safe) / safe)


def _m32_c(ell, sigma, dt):
    """models.py:61-73 for complex arguments (the complex step below), in forms whose real AND imaginary parts carry no cancellation.
    With x = 2 eta, eta = sqrt(3) dt / ell:
        Sigma[0] = sigma^2 (1 - exp(-x) (1 + x + x^2 / 2))                   = sigma^2 exp(-x) x^3 psi(x)
        Sigma[2] = gamma^2 sigma^2 (1 - exp(-x) (1 - x + x^2 / 2))           = gamma^2 sigma^2 exp(-x) (2 x + x^3 psi(x))
        F[0]     = (1 + eta) exp(-eta)                                       = 1 + eta^2 sum (-1)^k (-1 - k) / (k + 2)! eta^k
    psi(x) = sum x^k / (k + 3)! (positive terms): the series below x = 1 (eta = 0.5 for F[0]), the reference's closed form above, where its
    cancellation costs a factor of 12 at most.  (The primal -- csrc/cgp_models.hpp, models.py -- keeps the reference's formulas: the directions
    are the derivatives of the function those approximate to their own rounding.)"""
    gamma = np.sqrt(3.) / ell
    eta = dt * gamma
    x = 2 * eta
    e2 = np.exp(-x)
    beta = sigma ** 2 * e2
    e = np.exp(-eta)
    F = np.array([_below(eta, 0.5, 1. + eta * eta * _horner(eta, _F00), (1 + eta) * e), dt * e, -dt * gamma ** 2 * e, (1 - eta) * e])
    off = 2 * dt ** 2 * gamma ** 3 * beta
    tail = x ** 3 * _horner(x, _PSI)                                     # exp(x) - 1 - x - x^2 / 2
    S0 = _below(x, 1., beta * tail, sigma ** 2 - beta * (2 * eta + 2 * eta ** 2 + 1))
    S2 = gamma ** 2 * _below(x, 1., beta * (2 * x + tail), sigma ** 2 + beta * (2 * eta - 2 * eta ** 2 - 1))
    return F, np.array([S0, off, S2])


def _chirp_constants(p, dt, Xi):
    """The 24 model constants a tangent direction differentiates (include/chirpgp_hip.h: CGP_DIR_DOUBLES), as functions of the chirp
    builder's parameters lam, b, delta, ell, sigma, m0_v (models.py:437-459, 264-311, 56-58) -- complex-safe, vectorised over a
    trailing axis: p (6, G) -> (24, G).  q = b^2 (1 - exp(-2 lam dt)) / (2 lam) = b^2 dt phi(2 lam dt) with phi = _decay_ratio: one smooth
    function whose lam = 0 value is the reference's other branch, b^2 dt."""
    lam, b, delta, ell, sigma, m0_v = p
    q = b ** 2 * dt * _decay_ratio(2 * lam * dt)
    F, S = _m32_c(ell, sigma, dt)
    zero = 0. * lam
    P0 = [delta, zero, delta, zero, zero, sigma ** 2, zero, zero, zero, (np.sqrt(3.) / ell) ** 2 * sigma ** 2]
    return np.stack([-lam * dt, q, *F, *S, Xi + zero, zero, zero, m0_v, zero, *P0])


def _lascala_constants(p, dt, Xi):
    """models.py:497-519: delta, ell, sigma, m0_v; no damping, no chirp noise."""
    delta, ell, sigma, m0_v = p
    F, S = _m32_c(ell, sigma, dt)
    zero = 0. * delta
    P0 = [delta, zero, delta, zero, zero, sigma ** 2, zero, zero, zero, (np.sqrt(3.) / ell) ** 2 * sigma ** 2]
    return np.stack([zero, zero, *F, *S, Xi + zero, zero, zero, m0_v, zero, *P0])


def _constants_of(build):
    return {M.build_chirp_model: _chirp_constants, M.build_lascala_model: _lascala_constants}.get(build)


def tangent_directions(build, thetas, dt, Xi, h=1e-30):
    """d (model constants) / d theta_k for every row of thetas (G, P) -> (G, P, 24): complex-step derivatives of the builder's constants
    with respect to the positive parameters (exact to rounding), times d g(theta) / d theta = sigmoid(theta) (the reference's
    parametrisation, demos/ekfs_mle.py:39-47).

    The constants are differentiated in cancellation-free forms (_decay_ratio, _m32_c), not in the reference's: the complex step is exact
    for the formula it is given, its rounding included, and `1 - exp(-2 lam dt)` over `lam` or `sigma^2 - beta (2 eta + 2 eta^2 + 1)` lose
    every digit of their derivative for lam << 1 or a large ell (the lam-entry of d q was off by a factor of 27 at lam = 1e-6).  The primal
    -- the kernels' cgp_models.hpp, models.py, the checker's port -- keeps the reference's formulas for parity with it, so the gradient returned is
    the derivative of the function that primal approximates to its own rounding, not of the rounded formula.  Every entry is within 1e-12
    of the derivative taken in 100-digit arithmetic over lam 0 .. 10, b 1e-4 .. 10, ell 1e-2 .. 100, sigma 1e-2 .. 10
    (tests/test_gradient_directions.py).  At lam = 0 exactly (theta_lam -> -inf) d q / d lam is the limit -b^2 dt^2 and the entry is 0 with
    sigmoid(theta_lam)."""
    consts = _constants_of(build)
    thetas = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    G, P = thetas.shape
    out = np.empty((G, P, 24))
    with np.errstate(all='ignore'):
        params = np.logaddexp(0., thetas).T                      # (P, G): g(theta) to rounding (M.g's naive form is off by 1e-16 / g)
        dg = 1.0 / (1.0 + np.exp(-thetas))
        for k in range(P):
            pc = params.astype(np.complex128)
            pc[k] += 1j * h
            out[:, k, :] = (np.imag(consts(pc, dt, float(Xi))) / h).T * dg[:, k, None]
    return out


def _chirp_constants_cd(p, Xi):
    """The 27 constants of the CONTINUOUS model a tangent direction of cgp_cd_ekf_nll_grad differentiates (include/chirpgp_hip.h:
    CGP_CD_DIR_DOUBLES), as functions of the chirp builder's parameters lam, b, delta, ell, sigma, m0_v (models.py:437-459, 76-119):
    lam | gam = sqrt(3) / ell | gamma = b b^T = diag(b^2, b^2, 0, 4 sigma^2 gam^3), packed | Xi | m0 | P0, packed -- complex-safe,
    vectorised over a trailing axis: p (6, G) -> (27, G).  Products and powers only: nothing cancels, for any parameters."""
    lam, b, delta, ell, sigma, m0_v = p
    gam = np.sqrt(3.) / ell
    zero = 0. * lam
    Gam = [b ** 2, zero, b ** 2, zero, zero, zero, zero, zero, zero, 4. * sigma ** 2 * gam ** 3]
    P0 = [delta, zero, delta, zero, zero, sigma ** 2, zero, zero, zero, gam ** 2 * sigma ** 2]
    return np.stack([lam, gam, *Gam, Xi + zero, zero, zero, m0_v, zero, *P0])


def _lascala_constants_cd(p, Xi):
    """models.py:497-519, 181-261: delta, ell, sigma, m0_v; no damping, no chirp noise."""
    delta, ell, sigma, m0_v = p
    zero = 0. * delta
    return _chirp_constants_cd([zero, zero, delta, ell, sigma, m0_v], Xi)


def _constants_cd_of(build):
    return {M.build_chirp_model: _chirp_constants_cd, M.build_lascala_model: _lascala_constants_cd}.get(build)


def tangent_directions_cd(build, thetas, dt, Xi, h=1e-30):
    """tangent_directions for the continuous-discrete EKF (cgp_cd_ekf_nll_grad): d (constants of the continuous model) / d theta_k for every
    row of thetas (G, P) -> (G, P, 27), by complex step on _chirp_constants_cd / _lascala_constants_cd times sigmoid(theta).  The SDE's
    constants do not depend on dt (the kernel's RK4 stages take it as it is); the argument keeps the two functions' signatures alike.
    Every entry is within 1e-12 of the derivative taken in 100-digit arithmetic (tests/test_cd_gradient_host.py)."""
    consts = _constants_cd_of(build)
    thetas = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    G, P = thetas.shape
    out = np.empty((G, P, 27))
    with np.errstate(all='ignore'):
        params = np.logaddexp(0., thetas).T                      # (P, G): g(theta) to rounding, as in tangent_directions
        dg = 1.0 / (1.0 + np.exp(-thetas))
        for k in range(P):
            pc = params.astype(np.complex128)
            pc[k] += 1j * h
            out[:, k, :] = (np.imag(consts(pc, float(Xi))) / h).T * dg[:, k, None]
    return out


def _sigma_dim(sgps):
    xi = getattr(sgps, 'xi', None)
    return None if xi is None or np.ndim(xi) != 2 else int(np.shape(xi)[1])


def has_exact_gradient(method, build, Xi, sgps=None):
    """The in-kernel tangent gradient exists on the d = 4 chirp and La Scala models with a scalar Xi for the discrete EKF
    (cgp_ekf_nll_grad), for the continuous-discrete EKF (cgp_cd_ekf_nll_grad) and for the sigma-point filter with a d = 4 sigma-point
    set ``sgps`` (cgp_sgp_nll_grad).

    This predicate describes those three OLDER forms only, and its answers are held by tests/test_cd_gradient_host.py and
    tests/test_sgp_gradient_host.py, which assert False for 'cd_sgp_filter'.  The fourth form -- the continuous-discrete sigma-point
    filter's -- is built; :func:`has_tangent_kernel` is the predicate that says so, and the one every front end here goes by."""
    if _constants_of(build) is None or np.ndim(Xi) != 0:
        return False
    if method in ('ekf', 'cd_ekf'):
        return True
    return method == 'sgp_filter' and _sigma_dim(sgps) == 4


def has_tangent_kernel(method, build, Xi, sgps=None):
    """A tangent kernel -- value and exact gradient in one launch -- exists for ``method``: wherever has_exact_gradient says so, and for
    'cd_sgp_filter' on build_chirp_model / build_lascala_model with a scalar Xi and a d = 4 sigma-point set ``sgps`` (cgp_sgp_nll_grad on
    the SDE model: the tangent through the four RK4 stages of the sigma-point moment ODE).  value_and_grad, make_objective, fit and fit_many
    (exact=True) go by this predicate."""
    if has_exact_gradient(method, build, Xi, sgps):
        return True
    return method == 'cd_sgp_filter' and _constants_cd_of(build) is not None and np.ndim(Xi) == 0 and _sigma_dim(sgps) == 4


# Which form is the default (``exact=None``).  Measured on MI355X at T = 3141 (tools/grad_bench.py, profiles/r06_grad_bench.txt): the tangent
# kernel takes 3.7 - 4.4 ms per launch whatever the batch up to ~10 000 records (one lane per record and direction: a step is ~520
# dependent-issue vector instructions, 2800 cycles, and a wavefront issues them at the same rate for 6 lanes as for 64); the difference
# form runs 13 probes per record on the matrix-core EKF, 0.8 ms for one record, 0.94 ms for 64, 3.6 ms for 1000 and linear from there.
# So: exact where it is also the faster one -- from EXACT_FROM_RECORDS records in a launch -- and on request (exact=True) anywhere.
EXACT_FROM_RECORDS = 1500


def _exact_by_default(method, build, Xi, n_records, build_kw):
    return method == 'ekf' and has_exact_gradient(method, build, Xi) and not build_kw and n_records >= EXACT_FROM_RECORDS


def _exact_with_gaps(exact, missing):
    """``exact`` of an objective over records with gaps: the tangent kernels know no gaps (they take no flags, a NaN measurement
    propagates there), so missing='skip' resolves exact=None to the difference gradient and refuses exact=True."""
    from chirpgp_amd import _engine as E
    if not E._missing_flag(missing):
        return exact
    if exact:
        raise ValueError("exact=True does not go with missing='skip': the tangent kernels know no gaps (a NaN measurement propagates "
                         "through them); the difference gradient (exact=False, the default here) does")
    return False


def _exact_unsupported():
    return ValueError('exact=True: the tangent kernels are built for the discrete EKF, the continuous-discrete EKF and the sigma-point filters '
                      "('sgp_filter', 'cd_sgp_filter': with a d = 4 sigma-point set, sgps=) on build_chirp_model / build_lascala_model with a scalar Xi")


def _has_fisher_form(method):
    """The Fisher forms (cgp_ekf_nll_fisher, cgp_sgp_nll_fisher) exist for the discrete filters only."""
    return method not in ('cd_ekf', 'cd_sgp_filter')


def _fisher_unsupported(method):
    return ValueError(f'the tangent kernel of {method!r} writes value and gradient only: its Fisher form is not built '
                      '(value_grad_fisher, standard_errors and fit_scoring take the discrete EKF and the sigma-point filter)')


def _tangent_launch(fisher, build, thetas, ys, Xi, dt, record_index, method, sgps, missing=None, substeps=1):
    """One launch of a tangent kernel along tangent_directions at every row of thetas: (nll, grad) or, fisher, (nll, grad, F) as NumPy.
    ``missing='skip'``: NaN samples of the records are gaps (CGP_SKIP_MISSING: such a step adds exactly nothing to any of the three)."""
    from chirpgp_amd import _engine as E
    if not has_tangent_kernel(method, build, Xi, sgps):
        raise _exact_unsupported()
    if fisher and not _has_fisher_form(method):
        raise _fisher_unsupported(method)
    thetas = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    rows = _rows_per_record(thetas.shape[0], ys, record_index)
    with np.errstate(all='ignore'):
        drift, disp, disc, m0, P0, H = build(M.g(thetas))
    if method == 'cd_ekf':
        out = E.run_cd_ekf_nll_grad(drift, disp.outer(), H, Xi, m0, P0, dt, ys, tangent_directions_cd(build, thetas, dt, Xi),
                                    trials_per_record=rows, record_index=record_index, missing=missing, substeps=substeps)
        return tuple(o.cpu().numpy() for o in out)
    if method == 'cd_sgp_filter':
        out = E.run_cd_sgp_nll_grad(drift, disp.outer(), sgps, H, Xi, m0, P0, dt, ys, tangent_directions_cd(build, thetas, dt, Xi),
                                    trials_per_record=rows, record_index=record_index, missing=missing, substeps=substeps)
        return tuple(o.cpu().numpy() for o in out)
    dirs = tangent_directions(build, thetas, dt, Xi)
    if method == 'sgp_filter':
        out = (E.run_sgp_nll_fisher if fisher else E.run_sgp_nll_grad)(disc, sgps, H, Xi, m0, P0, dt, ys, dirs, trials_per_record=rows, record_index=record_index,
                                                                       missing=missing)
    else:
        out = (E.run_ekf_nll_fisher if fisher else E.run_ekf_nll_grad)(disc, H, Xi, m0, P0, dt, ys, dirs, trials_per_record=rows, record_index=record_index,
                                                                       missing=missing)
    return tuple(o.cpu().numpy() for o in out)


def value_and_grad(build, thetas, ys, Xi, dt, record_index=None, *, method='ekf', sgps=None, missing=None, substeps=1):
    """Objective and its EXACT gradient (forward tangents through the scan) at every row of thetas (G, P), in ONE launch: the EKF's
    (method='ekf', cgp_ekf_nll_grad: G P lanes), the continuous-discrete EKF's (method='cd_ekf', cgp_cd_ekf_nll_grad: G P lanes, the
    tangent carried through the four RK4 stages of every step), the sigma-point filter's (method='sgp_filter' with a d = 4 SigmaPoints
    ``sgps``, cgp_sgp_nll_grad: G wavefronts) or the continuous-discrete sigma-point filter's (method='cd_sgp_filter' with such a set: the
    same entry point on the SDE model, G wavefronts, the tangent through the four fans of every RK4 step).  ys (T,) or (R, T) shared out evenly over the rows as in batched_nll.  -> (nll (G,), grad (G, P)).
    ``missing='skip'``: NaN samples of the records are gaps, as in batched_nll -- the likelihood of the observed samples alone and its
    exact gradient; a record of NaN only gives 0 and a zero gradient.  ``substeps=n`` (method='cd_ekf', 'cd_sgp_filter'): n RK4 steps of dt / n between two
    measurements, as in batched_nll -- the tangent goes through every one of them."""
    _exact_with_substeps(True, method, substeps)
    return _tangent_launch(False, build, thetas, ys, Xi, dt, record_index, method, sgps, missing, substeps)


def value_grad_fisher(build, thetas, ys, Xi, dt, record_index=None, *, method='ekf', sgps=None, missing=None):
    """value_and_grad's results and, from the same launch, the Fisher information of the filter's Gaussian innovations model
    F[i][j] = sum_t (d nu_i d nu_j / S + d S_i d S_j / (2 S^2)) (cgp_ekf_nll_fisher, cgp_sgp_nll_fisher): the Gauss-Newton part of the NLL's
    Hessian, taken along tangent_directions -- the information in the UNCONSTRAINED theta.  Same eligibility and record addressing as
    value_and_grad.  -> (nll (G,), grad (G, P), fisher (G, P, P)); fisher is exactly symmetric.  ``missing='skip'``: the sum runs over the
    observed steps only -- the information of the observed samples; a record of NaN only gives F = 0."""
    return _tangent_launch(True, build, thetas, ys, Xi, dt, record_index, method, sgps, missing)


SINGULAR_RCOND = 1e-12       # covariance_from_fisher: below this 1 / cond of the scaled information, the estimate has a flat direction


def covariance_from_fisher(F, theta):
    """Standard errors from a Fisher information F (P, P) in the unconstrained theta (P,): pure NumPy.

    F is scaled by its diagonal, C = D^-1/2 F D^-1/2, so that the parameters' units do not decide its conditioning.  If C has no Cholesky
    factor or 1 / cond(C) < SINGULAR_RCOND the information is singular: singular = True and every entry is inf -- a pseudo-inverse would
    UNDERSTATE the uncertainty along a flat direction.  Otherwise cov_theta = F^-1 = D^-1/2 C^-1 D^-1/2 and the standard errors of the
    positive parameters g(theta) follow by the delta method through the reference's g (softplus, models.py:50):
    se_params = g'(theta) sqrt(diag cov_theta), g' = sigmoid.  -> (se_params (P,), cov_theta (P, P), cond, singular)."""
    F = np.asarray(F, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    P = theta.size
    if F.shape != (P, P):
        raise ValueError(f'F must be ({P}, {P}); got {F.shape}')
    flat = (np.full(P, np.inf), np.full((P, P), np.inf), np.inf, True)
    d = np.diag(F)
    if not np.all(np.isfinite(F)) or not np.all(d > 0):
        return flat
    s = 1.0 / np.sqrt(d)
    C = F * s[:, None] * s[None, :]
    C = 0.5 * (C + C.T)
    try:
        np.linalg.cholesky(C)
    except np.linalg.LinAlgError:
        return flat
    cond = float(np.linalg.cond(C))
    if not np.isfinite(cond) or 1.0 / cond < SINGULAR_RCOND:
        return flat[0], flat[1], cond, True
    cov = np.linalg.inv(C) * s[:, None] * s[None, :]
    cov = 0.5 * (cov + cov.T)
    with np.errstate(over='ignore'):
        dg = 1.0 / (1.0 + np.exp(-theta))
    return dg * np.sqrt(np.diag(cov)), cov, cond, False


def standard_errors(build, theta_hat, ys, Xi, dt, *, method='ekf', sgps=None, missing=None):
    """Standard errors of the fitted positive parameters g(theta_hat) of ONE record ys (T,) from the Fisher information at theta_hat (one
    launch of value_grad_fisher; covariance_from_fisher).  -> (se_params (P,), cov_theta (P, P), info) with info['fisher'], ['cond'],
    ['singular'], ['nll'] and ['grad']; a singular information gives inf everywhere and info['singular'] = True.  ``missing='skip'``: NaN
    samples are gaps and the information is the observed samples'; a record of NaN only has none (F = 0: singular)."""
    theta_hat = np.asarray(theta_hat, dtype=np.float64).reshape(-1)
    nll, grad, F = value_grad_fisher(build, theta_hat[None, :], ys, Xi, dt, method=method, sgps=sgps, missing=missing)
    se, cov, cond, singular = covariance_from_fisher(F[0], theta_hat)
    return se, cov, dict(fisher=F[0], cond=cond, singular=singular, nll=float(nll[0]), grad=grad[0])


def scoring_step(F, grad, mu):
    """The damped scoring step of fit_scoring, pure NumPy: (F + mu diag F) step = -grad.

    With mu > 0 and a positive semi-definite F the matrix is singular only where a diagonal entry of F is exactly 0, and then that
    parameter's whole row and column are 0: the likelihood does not see it along these directions (lam = 0, or a chirp noise b that has
    underflowed).  Such a parameter STAYS WHERE IT IS (step 0, whatever its gradient entry) and the others take the step of the system
    without it, which is positive definite.  -> step (P,)."""
    F, grad = np.asarray(F, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    seen = np.diag(F) > 0
    step = np.zeros(grad.size)
    if seen.any():
        A = F[np.ix_(seen, seen)]
        step[seen] = np.linalg.solve(A + mu * np.diag(np.diag(A)), -grad[seen])
    return step


def fit_scoring(method, build, init_params, yss, Xi, dt, sgps=None, maxiter=100, gtol=1e-5, mu0=1e-3, nu=4.0, mu_max=1e12, *, missing=None):
    """Maximum likelihood for R records in lock step by damped Fisher scoring: every iteration is ONE launch of value_grad_fisher for all
    the records still active, each with its own iterate and damping.  A tangent launch costs the same whatever the batch
    (EXACT_FROM_RECORDS), so the launches are the cost; scoring uses the curvature the kernel already carries instead of building it up
    from gradient differences as fit_many's L-BFGS does.

    Step: (F + mu diag F) step = -grad.  It is accepted only if the NLL decreases (a non-finite trial value is a rejection); then
    mu /= nu, else mu *= nu, from mu = mu0.  A record leaves the active set when max |grad| <= gtol max(1, |f|) or when mu exceeds
    mu_max (no decrease along any damped direction).  The methods with a Fisher form only: 'ekf' and 'sgp_filter'.

    yss (R, T); init_params (P,) or (R, P) positive model parameters -> (opt_params (R, P), info): fit_many's fun, grad, nit, launches,
    converged (by the gradient rule), and fisher (R, P, P) at the final iterates, mu (R,), and per launch history (the (R,) NLLs of the
    iterates after it) and iterates (those iterates, (R, P), in the unconstrained theta = g_inv(params)).

    ``missing='skip'``: NaN samples of the records are gaps -- value, exact gradient and information of the observed samples, from the same
    launches (the L-BFGS front ends fit, fit_many and make_objective still take the difference gradient on such records)."""
    from chirpgp_amd import _engine as E
    if not has_tangent_kernel(method, build, Xi, sgps):
        raise _exact_unsupported()
    if not _has_fisher_form(method):
        raise _fisher_unsupported(method)
    E._missing_flag(missing)                           # a misspelt value fails here, before anything is copied
    yss = E.dev(yss)
    if yss.ndim == 1:
        yss = yss[None, :]
    R = yss.shape[0]
    x = np.array(np.broadcast_to(M.g_inv(np.asarray(init_params, dtype=np.float64)), (R, np.shape(init_params)[-1])))
    P = x.shape[1]

    def evaluate(xt, idx):
        ft, gt, Ft = value_grad_fisher(build, xt, yss, Xi, dt, record_index=idx, method=method, sgps=sgps, missing=missing)
        ok = np.isfinite(ft) & np.isfinite(gt).all(axis=1) & np.isfinite(Ft).all(axis=(1, 2))
        return np.where(ok, ft, np.inf), gt, Ft, ok

    f, g, F, ok = evaluate(x, None)
    launches = 1
    mu = np.full(R, float(mu0))
    nit = np.zeros(R, dtype=int)
    stalled = ~ok                                      # a start at which the filter diverges stays where it is

    def small(f_, g_):
        return np.abs(g_).max(axis=1) <= gtol * np.maximum(1.0, np.abs(f_))

    converged = ok & small(np.where(ok, f, 0.0), np.where(ok[:, None], g, 0.0))
    history, iterates = [f.copy()], [x.copy()]         # every record's NLL and iterate after every launch
    for _ in range(maxiter):
        active = ~(converged | stalled)
        if not active.any():
            break
        idx = np.flatnonzero(active)
        xt = x[idx].copy()
        for n, r in enumerate(idx):
            xt[n] += scoring_step(F[r], g[r], mu[r])
        with np.errstate(all='ignore'):
            ft, gt, Ft, okt = evaluate(xt, idx)
        launches += 1
        acc = okt & (ft < f[idx])
        a = idx[acc]
        x[a], f[a], g[a], F[a] = xt[acc], ft[acc], gt[acc], Ft[acc]
        nit[a] += 1
        mu[a] /= nu
        mu[idx[~acc]] *= nu
        converged[a] = small(f[a], g[a])
        stalled |= active & (mu > mu_max)
        history.append(f.copy())
        iterates.append(x.copy())
    return M.g(x), dict(fun=f, grad=g, nit=nit, launches=launches, converged=converged, fisher=F, mu=mu, history=history, iterates=iterates)


def make_objective(method, build, ys, Xi, dt, sgps=None, rel_step=1e-6, exact=None, *, missing=None, substeps=1, dts=None, **build_kw):
    """-> fun(theta) returning (nll, gradient): value and central differences from one batched launch of 2 P + 1 filter passes, or --
    ``exact=True``, the discrete EKF, the continuous-discrete EKF ('cd_ekf') or a sigma-point filter ('sgp_filter', 'cd_sgp_filter', with a
    d = 4 ``sgps``) on the chirp / La Scala models (has_tangent_kernel) -- value and EXACT
    gradient from one launch of a tangent kernel (cgp_ekf_nll_grad: within 8e-13 of the gradient's scale against 100-digit arithmetic where
    the differences carry 2e-7; slower for a single record, see EXACT_FROM_RECORDS; cgp_sgp_nll_grad).  exact=None takes the tangent kernel
    for the EKF from EXACT_FROM_RECORDS records only and never for the sigma-point filters.  ``missing='skip'`` (a record with gaps):
    differences only.  ``substeps=n`` ('cd_ekf', 'cd_sgp_filter'): n RK4 steps of dt / n between two measurements, in either form of the
    gradient (both have the exact one).  ``dts=`` ('cd_ekf', 'cd_sgp_filter'; dt is then None): one interval per step -- differences only,
    exact=None resolves to False and exact=True is refused (the tangent kernels take one dt)."""
    exact = _exact_with_times(_exact_with_substeps(_exact_with_gaps(exact, missing), method, substeps), method, dts, dt)
    if dts is not None:                               # checked once, here: every launch of the search passes the same intervals
        from chirpgp_amd import _engine as E
        shape = E._leading_shape(ys)
        E.check_intervals(dts, shape[-1], None if len(shape) == 1 else shape[0])
    if exact is None:
        exact = _exact_by_default(method, build, Xi, 1, build_kw)
    if exact:
        if not has_tangent_kernel(method, build, Xi, sgps) or build_kw:
            raise _exact_unsupported()
        from chirpgp_amd import _engine as E
        ys_dev = E.dev(ys)

        def fun_exact(theta):
            f, g_ = value_and_grad(build, np.asarray(theta, dtype=np.float64)[None, :], ys_dev, Xi, dt, method=method, sgps=sgps, substeps=substeps)
            if not np.isfinite(f[0]):                   # diverged filter: the reference writes NaN results and moves on
                return np.inf, np.zeros(np.size(theta))
            return float(f[0]), np.where(np.isfinite(g_[0]), g_[0], 0.0)
        return fun_exact

    def fun(theta):
        theta = np.asarray(theta, dtype=np.float64)
        P = theta.size
        h = rel_step * (1.0 + np.abs(theta))
        batch = np.tile(theta, (2 * P + 1, 1))
        for i in range(P):
            batch[1 + 2 * i, i] += h[i]
            batch[2 + 2 * i, i] -= h[i]
        nll = batched_nll(method, build, batch, ys, Xi, dt, sgps, missing=missing, substeps=substeps, dts=dts, check_dts=False, **build_kw)
        grad = (nll[1::2] - nll[2::2]) / (2 * h)
        f = float(nll[0])
        if not np.isfinite(f):                      # diverged filter: the reference writes NaN results and moves on
            return np.inf, np.zeros(P)
        return f, np.where(np.isfinite(grad), grad, 0.0)
    return fun


# L-BFGS-B's stopping rule where the gradient is differenced from the filter's NLL (see fit; tests/test_mle_stopping_rule.py)
DIFFERENCE_STOP = dict(ftol=1e-13, gtol=1e-7)


def fit(method, build, init_params, ys, Xi, dt, sgps=None, maxiter=200, exact=None, *, missing=None, substeps=1, dts=None, **build_kw):
    """L-BFGS-B from ``init_params`` (positive model parameters, e.g. [0.1, 0.1, 0.1, 1, 1, 7]).
    Returns (opt_params, scipy OptimizeResult).

    With the difference form of the gradient the stopping rule is tighter than SciPy's default (ftol 2.2e-9, gtol 1e-5).  These
    likelihoods end in a shallow valley, and under the default rule the point at which the search stops is decided by the last bits of
    the filter's NLL, which the differences amplify: on a T = 3141 chirp record, perturbing the NLL by 2e-14 of its value (a few units in
    the last place, what any re-ordering of the filter's arithmetic does) moved the parameters at which it stopped by up to 2.2e-3 of
    their value, seven runs, although every NLL agreed to 1e-7.  With ftol 1e-13 and gtol 1e-7 the same seven runs end within 1.7e-4 of
    the optimum, for 60 - 85 objective launches where the default took 45 - 55.  (The tangent kernels' searches, exact=True, keep
    SciPy's rule.)  ``substeps`` and ``dts`` as in :func:`make_objective`."""
    from scipy.optimize import minimize
    exact = _exact_with_times(_exact_with_substeps(_exact_with_gaps(exact, missing), method, substeps), method, dts, dt)
    if exact is None:
        exact = _exact_by_default(method, build, Xi, 1, build_kw)
    fun = make_objective(method, build, ys, Xi, dt, sgps, exact=exact, missing=missing, substeps=substeps, dts=dts, **build_kw)
    stop = {} if exact else DIFFERENCE_STOP
    res = minimize(fun, M.g_inv(np.asarray(init_params, dtype=np.float64)), jac=True, method='L-BFGS-B',
                   options=dict(maxiter=maxiter, **stop))
    return M.g(res.x), res


def _value_and_grad_many(method, build, thetas, yss, Xi, dt, sgps, rel_step, build_kw, record_index=None, exact=None, missing=None, substeps=1,
                         dts=None):
    """NLL and gradient of R records (the rows ``record_index`` of yss; all of them by default) at R parameter vectors: exact (the tangent
    kernel, R P lanes) for the discrete EKF on the chirp / La Scala models (and, with exact=True, the sigma-point filter's, R wavefronts),
    else central differences -- ONE launch of R (2 P + 1) trials, each record read in place by its 2 P + 1 probes."""
    R, P = thetas.shape
    exact = _exact_with_times(_exact_with_substeps(_exact_with_gaps(exact, missing), method, substeps), method, dts, dt)
    if exact is None:
        exact = _exact_by_default(method, build, Xi, R, build_kw)
    if exact:
        if not has_tangent_kernel(method, build, Xi, sgps) or build_kw:
            raise _exact_unsupported()
        f, grad = value_and_grad(build, thetas, yss, Xi, dt, record_index=record_index, method=method, sgps=sgps, substeps=substeps)
        f = f.copy()
        f[~np.isfinite(f)] = np.inf
        return f, np.where(np.isfinite(grad), grad, 0.0)
    h = rel_step * (1.0 + np.abs(thetas))                                   # (R, P)
    batch = np.repeat(thetas[:, None, :], 2 * P + 1, axis=1)                # (R, 2P+1, P)
    idx = np.arange(P)
    batch[:, 1 + 2 * idx, idx] += h
    batch[:, 2 + 2 * idx, idx] -= h
    nll = batched_nll(method, build, batch.reshape(-1, P), yss, Xi, dt, sgps, record_index=record_index, missing=missing, substeps=substeps,
                      dts=dts, check_dts=False, **build_kw).reshape(R, 2 * P + 1)      # (fit_many has checked the intervals)
    f = nll[:, 0].copy()
    grad = (nll[:, 1::2] - nll[:, 2::2]) / (2 * h)
    f[~np.isfinite(f)] = np.inf
    return f, np.where(np.isfinite(grad), grad, 0.0)


def fit_many(method, build, init_params, yss, Xi, dt, sgps=None, maxiter=200, history=10, gtol=1e-5, ftol=2.2e-9,
             rel_step=1e-6, exact=None, *, missing=None, substeps=1, dts=None, **build_kw):
    """Maximum likelihood for R measurement records in lock step: limited-memory BFGS with a backtracking (Armijo) line
    search, every record with its own iterate, history and step length, and every probe of every record evaluated in
    the SAME kernel launch (R x 13 trials for the chirp model).  A launch costs T x 0.35 us whatever the batch up to
    ~4000 trials, so R records take the wall time of one -- the reference's Monte-Carlo jobs (tetralith/jobs/*_mle.py)
    run one L-BFGS-B per record.  Same objective, same unconstrained parametrisation g() as :func:`fit`.

    yss (R, T);  init_params (P,) or (R, P) positive model parameters  ->  (opt_params (R, P), info dict).
    ``missing='skip'``: NaN samples of the records are gaps (difference gradient only, as in :func:`make_objective`); ``substeps`` likewise;
    ``dts=`` (dt then None): (T,) one time grid for all records or (R, T) one per record, difference gradient only."""
    from chirpgp_amd import _engine as E
    _substeps_kw(method, substeps)                    # a count or a method that cannot take it fails here, before anything is copied
    exact = _exact_with_times(exact, method, dts, dt)
    if dts is not None:                               # checked once, on the host: every launch of the search passes the same grids
        shape = E._leading_shape(yss)
        dts = E.check_intervals(dts, shape[-1], None if len(shape) == 1 else shape[0])
        dts = dts[0] if dts.shape[0] == 1 else dts
    yss = E.dev(yss)                                 # uploaded once; every probe of every line search reads it in place
    if yss.ndim == 1:
        yss = yss[None, :]
    R = yss.shape[0]
    x = np.array(np.broadcast_to(M.g_inv(np.asarray(init_params, dtype=np.float64)), (R, np.shape(init_params)[-1])))
    P = x.shape[1]
    f, g = _value_and_grad_many(method, build, x, yss, Xi, dt, sgps, rel_step, build_kw, exact=exact, missing=missing, substeps=substeps, dts=dts)
    S, Y = [], []                                    # lists of (R, P) pairs, newest last
    done = ~np.isfinite(f)
    nit = np.zeros(R, dtype=int)
    launches = 1
    for _ in range(maxiter):
        if done.all():
            break
        # two-loop recursion, vectorised over the records; pairs with s . y <= 0 carry rho = 0 and drop out
        q = g.copy()
        alphas = []
        for s_, y_ in zip(reversed(S), reversed(Y)):
            sy = np.einsum('rp,rp->r', s_, y_)
            rho = np.where(sy > 1e-300, 1.0 / np.where(sy > 1e-300, sy, 1.0), 0.0)
            a = rho * np.einsum('rp,rp->r', s_, q)
            q -= a[:, None] * y_
            alphas.append((a, rho))
        if S:
            sy = np.einsum('rp,rp->r', S[-1], Y[-1]); yy = np.einsum('rp,rp->r', Y[-1], Y[-1])
            q *= np.where((sy > 1e-300) & (yy > 0), sy / np.where(yy > 0, yy, 1.0), 1.0)[:, None]
        for (a, rho), s_, y_ in zip(reversed(alphas), S, Y):
            b = rho * np.einsum('rp,rp->r', y_, q)
            q += (a - b)[:, None] * s_
        d = -q
        gd = np.einsum('rp,rp->r', g, d)
        bad = ~(gd < 0)                               # not a descent direction (or NaN): steepest descent
        d[bad] = -g[bad]; gd[bad] = -np.einsum('rp,rp->r', g[bad], g[bad])
        step = np.ones(R) if S else np.minimum(1.0, 1.0 / np.maximum(np.abs(g).sum(axis=1), 1e-300))
        searching = ~done
        x_new, f_new, g_new = x.copy(), f.copy(), g.copy()
        for _ls in range(25):
            if not searching.any():
                break
            idx = np.flatnonzero(searching)
            xt = x[idx] + step[idx, None] * d[idx]
            ft, gt = _value_and_grad_many(method, build, xt, yss, Xi, dt, sgps, rel_step, build_kw, record_index=idx, exact=exact, missing=missing,
                                          substeps=substeps, dts=dts)
            launches += 1
            ok = ft <= f[idx] + 1e-4 * step[idx] * gd[idx]
            acc = idx[ok]
            x_new[acc], f_new[acc], g_new[acc] = xt[ok], ft[ok], gt[ok]
            searching[acc] = False
            step[idx[~ok]] *= 0.5
        failed = searching.copy()                     # line search exhausted: this record stops where it is
        moved = ~done & ~failed
        s_, y_ = x_new - x, g_new - g
        s_[~moved] = 0.0; y_[~moved] = 0.0
        S.append(s_); Y.append(y_)
        if len(S) > history:
            S.pop(0); Y.pop(0)
        small = (f - f_new) <= ftol * np.maximum(np.maximum(np.abs(f), np.abs(f_new)), 1.0)
        x, f, g = x_new, f_new, g_new
        nit[moved] += 1
        done |= failed | (moved & (small | (np.abs(g).max(axis=1) <= gtol)))
    return M.g(x), dict(fun=f, grad=g, nit=nit, launches=launches, converged=done)


def grid_search(method, build, grid, yss, Xi, dt, sgps=None, *, substeps=1, dts=None, **build_kw):
    """Parameter-grid MLE sweep (BASELINE config C5: "batch x param-grid MLE sweep"): the final NLL of ``method`` at every
    grid point for every record, in ONE launch of R G trials -- G parameter vectors per record, each record read in place.

    grid (G, P) positive model parameters; yss (R, T) or (T,)  ->  (best (R, P), nll (R, G), argmin (R,)).
    A diverged grid point (NaN / inf NLL) never wins; a record whose every grid point diverges gets NaN parameters.
    ``dts=`` ('cd_ekf', 'cd_sgp_filter'; dt then None): one interval per step, (T,) or one time grid per record."""
    grid = np.atleast_2d(np.asarray(grid, dtype=np.float64))
    G = grid.shape[0]
    R = 1 if np.ndim(yss) == 1 else int(np.shape(yss)[0])
    thetas = np.tile(M.g_inv(grid), (R, 1))                     # record-major: the G rows of a record are consecutive trials
    nll = batched_nll(method, build, thetas, yss, Xi, dt, sgps, substeps=substeps, dts=dts, **build_kw).reshape(R, G)
    masked = np.where(np.isfinite(nll), nll, np.inf)
    arg = np.argmin(masked, axis=1)
    best = M.g(M.g_inv(grid))[arg]                              # the parameters the filter actually ran with
    best[~np.isfinite(masked[np.arange(R), arg])] = np.nan
    return best, nll, arg
