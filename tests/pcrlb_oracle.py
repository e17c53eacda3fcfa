"""Float64 NumPy restatement of the posterior Cramer-Rao blocks (chirpgp_amd/csrc/cgp_pcrlb.hpp, "THE MATHEMATICS"), one sample at a
time and with dense matrices throughout: no entry is treated as a constant of the model, nothing is shared with the kernel's block
forms.  TEST INFRASTRUCTURE (a helper like tests/sample_oracle.py), checked itself against 100-digit arithmetic
(tests/golden/exact_pcrlb.npz, written by tests/golden/make_exact_pcrlb.py, which shares no code with this file).

For one pair (x_s, x_t):   P = Sigma^-1,  J = dm/dx at x_s,  r = x_t - m(x_s),  w = P r,
    b11 = J^T P J - sum_i w_i Hess m_i(x_s),      b12 = -J^T P   (index [s][t]),      D22 = P + H H^T / Xi.
"""
import math

import numpy as np

M_LINEAR, M_HARMONIC_LCD = 0, 1

# The oracle's own error against the 100-digit fixture, per model and array: max |difference| / the array's largest entry, measured
# by tests/test_pcrlb_host.py on the CPU and recorded here ROUNDED UP to the next power of ten.  These are the oracle's gates; the
# kernel's gate on the GPU is 10 x the larger of a model's two block figures (kernel_gate).  'recursion' is chirpgp_amd.crlb.recursion
# fed the fixture's exact blocks: its D22 comes from the descriptor's float64 covariance while the blocks are exact, so the rounding of
# Sigma^-1 does not cancel in the Schur complement as it does in 'js', where the oracle's blocks and its D22 share it.
# Measured (x86-64):                 b11        b12        js         recursion
#     chirp (d = 4, dt = 0.05)       5.90e-13   6.08e-13   8.49e-15   3.20e-11
#     nh2   (d = 6, dt = 0.1)        1.22e-13   1.32e-13   3.75e-15   4.21e-12
#     nh3   (d = 8, dt = 0.1)        8.49e-14   9.12e-14   1.29e-14   6.54e-12
#     m32   (d = 2, dt = 0.1)        1.61e-16   3.22e-16   2.12e-15   4.40e-15
# The harmonic models' figures are the cancellation in the closed form of the Matern block of Sigma (models.py:61-73: a difference of
# O(1) terms that leaves O((dt / ell)^3)), which the 100-digit side does not suffer; the linear model is handed Sigma as numbers.
ORACLE_ERROR = {
    'chirp': {'b11': 1e-12, 'b12': 1e-12, 'js': 1e-14, 'recursion': 1e-10},
    'nh2': {'b11': 1e-12, 'b12': 1e-12, 'js': 1e-14, 'recursion': 1e-11},
    'nh3': {'b11': 1e-13, 'b12': 1e-13, 'js': 1e-13, 'recursion': 1e-11},
    'm32': {'b11': 1e-15, 'b12': 1e-15, 'js': 1e-14, 'recursion': 1e-14},
}


def kernel_gate(name):
    """The GPU gate of one model: 10 x the oracle's recorded error on the blocks."""
    return 10.0 * max(ORACLE_ERROR[name]['b11'], ORACLE_ERROR[name]['b12'])


def _softplus3(v):
    """g, g', g'' = g' (1 - g') of the softplus, in the naive form of models.py:50 (its derivative written so that exp's overflow is 1)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp(v)
        g = np.log(e + 1.0)
        d1 = np.where(np.isinf(e), 1.0, e / (e + 1.0))
    return g, d1, d1 * (1.0 - d1)


def _m32(ell, sigma, dt):
    gam = math.sqrt(3.0) / ell
    eta = dt * gam
    beta = sigma ** 2 * math.exp(-2 * eta)
    F = np.array([[1 + eta, dt], [-dt * gam ** 2, 1 - eta]]) * math.exp(-eta)
    off = 2 * dt ** 2 * gam ** 3 * beta
    S = np.array([[sigma ** 2 - beta * (2 * eta + 2 * eta ** 2 + 1), off],
                  [off, gam ** 2 * (sigma ** 2 + beta * (2 * eta - 2 * eta ** 2 - 1))]])
    return F, S


def sigma_of(model_id, d, params, dt):
    params = np.asarray(params, dtype=np.float64)
    if model_id == M_LINEAR:
        return params[d * d:].reshape(d, d)
    lam, b, ell, sigma, _ = params
    q = b * b * dt if lam == 0.0 else b * b / (2 * lam) * (1 - math.exp(-2 * lam * dt))
    S = np.zeros((d, d))
    S[np.arange(d - 2), np.arange(d - 2)] = q
    S[d - 2:, d - 2:] = _m32(ell, sigma, dt)[1]
    return S


def precision_of(model_id, d, params, dt):
    S = sigma_of(model_id, d, params, dt)
    try:
        np.linalg.cholesky(S)
        return np.linalg.inv(S)
    except np.linalg.LinAlgError:
        return np.full((d, d), np.nan)


def mean_jac_hess(model_id, d, params, dt, u):
    """m(u) (..., d), J (..., d, d), and Hess m_i stacked (..., d, d, d), for one state or a stack of states (every state on its own:
    the leading axes only save Python loops)."""
    params = np.asarray(params, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    lead = u.shape[:-1]
    hess = np.zeros(lead + (d, d, d))
    if model_id == M_LINEAR:
        F = params[:d * d].reshape(d, d)
        return u @ F.T, np.broadcast_to(F, lead + (d, d)).copy(), hess
    lam, _, ell, sigma, fs = params
    nh, iv = (d - 2) // 2, d - 2
    rho = math.exp(-lam * dt)
    g, g1, g2 = _softplus3(u[..., iv])
    base = dt * 2 * math.pi * fs
    m, J = np.zeros(lead + (d,)), np.zeros(lead + (d, d))
    for k in range(nh):
        th, th1, th2 = (k + 1) * base * g, (k + 1) * base * g1, (k + 1) * base * g2
        c, s = rho * np.cos(th), rho * np.sin(th)
        a, b = 2 * k, 2 * k + 1
        m[..., a], m[..., b] = c * u[..., a] - s * u[..., b], s * u[..., a] + c * u[..., b]
        J[..., a, a], J[..., a, b], J[..., b, a], J[..., b, b] = c, -s, s, c
        J[..., a, iv], J[..., b, iv] = -th1 * m[..., b], th1 * m[..., a]
        hess[..., a, a, iv] = hess[..., a, iv, a] = -th1 * s
        hess[..., a, b, iv] = hess[..., a, iv, b] = -th1 * c
        hess[..., a, iv, iv] = -th2 * m[..., b] - th1 * th1 * m[..., a]
        hess[..., b, a, iv] = hess[..., b, iv, a] = th1 * c
        hess[..., b, b, iv] = hess[..., b, iv, b] = -th1 * s
        hess[..., b, iv, iv] = th2 * m[..., a] - th1 * th1 * m[..., b]
    Fm = _m32(ell, sigma, dt)[0]
    m[..., iv:] = u[..., iv:] @ Fm.T
    J[..., iv:, iv:] = Fm
    return m, J, hess


def second_order(model_id, d, params, dt, P, xs, xt):
    """sum_i w_i Hess m_i(x_s), w = P (x_t - m(x_s))."""
    m, _, hess = mean_jac_hess(model_id, d, params, dt, xs)
    w = (np.asarray(xt, dtype=np.float64) - m) @ P.T
    return np.einsum('...i,...ijk->...jk', w, hess)


def pair_blocks(model_id, d, params, dt, xs, xt, P=None):
    """(b11, b12) of one pair -- or of a stack of pairs --, dense (..., d, d) each."""
    if P is None:
        P = precision_of(model_id, d, params, dt)
    _, J, _ = mean_jac_hess(model_id, d, params, dt, xs)
    Jt = np.swapaxes(J, -1, -2)
    return Jt @ P @ J - second_order(model_id, d, params, dt, P, xs, xt), -(Jt @ P)


def pack(b11, b12):
    """(..., d, d) blocks -> (..., K) rows in cgp_pcrlb_sums' order: packed lower triangle of b11 (00 10 11 20 ...), then b12 row-major."""
    d = b11.shape[-1]
    il = np.tril_indices(d)
    return np.concatenate([b11[..., il[0], il[1]], b12.reshape(b12.shape[:-2] + (d * d,))], axis=-1)


def sums(model_id, d, params, dt, x0, xs):
    """(K, T): the sums over the trials of x0 (B, d), xs (B, T, d), every sample evaluated on its own (a slab of trials per call)."""
    x0, xs = np.asarray(x0, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    B, T = xs.shape[:2]
    P = precision_of(model_id, d, params, dt)
    prev = np.concatenate([x0[:, None, :], xs[:, :-1]], axis=1)
    rows = np.empty((B, T, d * (d + 1) // 2 + d * d))
    step = max(1, 4096 // max(T, 1))
    for lo in range(0, B, step):
        rows[lo:lo + step] = pack(*pair_blocks(model_id, d, params, dt, prev[lo:lo + step], xs[lo:lo + step], P))
    # the sum over the trials correctly rounded (math.fsum): a running float64 sum of 1000 equal terms is itself off by 1e-14 of its value
    return np.array([[math.fsum(rows[:, t, k]) for t in range(T)] for k in range(rows.shape[2])])


def d22(model_id, d, params, dt, H, Xi):
    H = np.asarray(H, dtype=np.float64)
    return precision_of(model_id, d, params, dt) + np.outer(H, H) / Xi


def recursion(d11, d12, d22_, j0):
    """J_t = D22 - D12_t^T (J_{t-1} + D11_t)^-1 D12_t over the leading axis of d11 / d12; not symmetrised."""
    j, out = np.array(j0, dtype=np.float64), []
    for a, b in zip(d11, d12):
        j = d22_ - b.T @ np.linalg.solve(j + a, b)
        out.append(j)
    return np.array(out)
