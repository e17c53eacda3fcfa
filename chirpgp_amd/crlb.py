"""Posterior Cramer-Rao lower bound of the discrete models (chirpgp/models.py:583-644, Tichavsky's recursion with Monte-Carlo
expectations), for the models this engine enumerates: a Gaussian transition with a constant covariance and a linear measurement.

The Monte-Carlo part -- the sums over the trials of the per-sample blocks D11 and D12 -- is a kernel of the engine
(include/chirpgp_hip.h: cgp_pcrlb_sums; the mathematics is written out in csrc/cgp_pcrlb.hpp).  What is left is T solves of d x d,
host NumPy like the optimisers of mle.py:

    sums = crlb.sums(cond_m_cov, dt, x0, xs)               # (K, T) on the device; pass sums= to accumulate chunk by chunk
    js = crlb.recursion(sums, n, j0, cond_m_cov, H, Xi, dt)    # (T, d, d): the information matrices J_1 .. J_T
    Ps = crlb.bound(js)                                    # their inverses: the bound on any estimator's error covariance
"""
import numpy as np

__all__ = ['sums', 'unpack', 'recursion', 'bound']


def _descriptor(cond_m_cov, dt):
    from chirpgp_amd import _engine as E
    from chirpgp_amd import models as M
    spec = cond_m_cov
    if hasattr(spec, 'at') and not isinstance(spec, M.DiscreteModel):
        spec = spec.at(dt)
    if isinstance(spec, M.DriftModel):
        raise ValueError(f'the posterior Cramer-Rao sums take a discrete (cond_m_cov) model, not the SDE drift {spec!r}: discretise it first')
    if isinstance(spec, M._CustomSpec):
        raise ValueError(f'the posterior Cramer-Rao sums need the Hessian of the model\'s mean, which a run-time compiled model ({spec!r}) does not state')
    if not isinstance(spec, M.DiscreteModel):
        raise TypeError('cond_m_cov must be a chirpgp_amd.models discrete descriptor (disc_chirp_lcd(...), disc_harmonic_chirp_lcd(...), '
                        'linear_cond_m_cov(F, Sigma)); arbitrary Python callables cannot run inside the HIP kernels')
    if spec.model_id == E.M_LASCALA_LCD:
        raise ValueError('disc_model_lascala_lcd has a singular transition covariance (its chirp states carry no noise): '
                         'the transition has no density and the bound is not defined')
    if spec.model_id not in (E.M_LINEAR, E.M_HARMONIC_LCD):
        raise ValueError(f'the posterior Cramer-Rao sums take linear_cond_m_cov and the harmonic chirp LCD models, not {spec!r}')
    return spec


def sums(cond_m_cov, dt, x0, xs, sums=None):
    """The (K, T) device tensor of cgp_pcrlb_sums, K = d (d + 1) / 2 + d d, over the trials x0 (B, d), xs (B, T, d); `sums`: a tensor of
    an earlier chunk to add into.  Divide by the number of trials (after the all-reduce over ranks) for the means."""
    from chirpgp_amd import _engine as E
    return E.run_pcrlb_sums(_descriptor(cond_m_cov, dt), dt, x0, xs, sums=sums)


def unpack(sums, n, d):
    """(K, T) sums over n trials -> D11 (T, d, d) (symmetric, from its packed lower triangle) and D12 (T, d, d), index [s][t]."""
    a = sums.detach().cpu().numpy() if hasattr(sums, 'detach') else np.asarray(sums, dtype=np.float64)
    n11 = d * (d + 1) // 2
    if a.ndim != 2 or a.shape[0] != n11 + d * d:
        raise ValueError(f'sums must be ({n11 + d * d}, T) for d = {d}; got {a.shape}')
    a = a / float(n)
    T = a.shape[1]
    d11 = np.empty((T, d, d))
    il = np.tril_indices(d)                                 # row-major lower triangle: 00 10 11 20 21 22 ...
    d11[:, il[0], il[1]] = a[:n11].T
    d11[:, il[1], il[0]] = a[:n11].T
    return d11, a[n11:].T.reshape(T, d, d).copy()


def recursion(sums, n, j0, cond_m_cov, H, Xi, dt):
    """J_t = D22 - D12_t^T (J_{t-1} + D11_t)^-1 D12_t, J_0 = j0 (models.py:632-643; not symmetrised, as there) -> js (T, d, d), NumPy.
    D22 = Sigma^-1 + H H^T / Xi is constant and comes from the descriptor's own host covariance."""
    spec = _descriptor(cond_m_cov, dt)
    d = spec.d
    j = np.array(j0, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64).reshape(-1)
    if j.shape != (d, d) or H.shape != (d,):
        raise ValueError(f'j0 must be ({d}, {d}) and H ({d},); got {j.shape}, {H.shape}')
    d11, d12 = unpack(sums, n, d)
    _, cov = spec(np.zeros(d), dt)
    with np.errstate(all='ignore'):
        try:
            d22 = np.linalg.inv(cov) + np.outer(H, H) / float(Xi)
        except np.linalg.LinAlgError:
            d22 = np.full((d, d), np.nan)
    js = np.empty((d11.shape[0], d, d))
    for t in range(d11.shape[0]):
        try:
            j = d22 - d12[t].T @ np.linalg.solve(j + d11[t], d12[t])
        except np.linalg.LinAlgError:                       # jnp.linalg.solve returns NaN / inf instead of raising
            j = np.full((d, d), np.nan)
        js[t] = j
    return js


def bound(js):
    """The lower bound itself: inv(J_t) for every t."""
    return np.linalg.inv(np.asarray(js, dtype=np.float64))
