"""The continuous-discrete EKF's final NLL and its exact gradient in float64 NumPy: a forward-tangent restatement of the recursion, written
from the formulas and not from the kernel (csrc/cgp_tangent4_cd.hpp) -- dense 4 x 4 matrices, every direction at once, the derivatives of
the model's constants taken analytically (the kernel's host side takes them by complex step).  tests/test_cd_gradient_host.py holds it
against the 100-digit fixture: float64 reaches the gates before the GPU is asked to.

    cd_ekf (filters_smoothers.py:352-397):  per measurement one RK4 step (quadratures.py:34-54) of
        dm/dt = a(m),   dP/dt = J P + P J^T + Gamma
    then the scalar update (filters_smoothers.py:55-68).  Chirp SDE (models.py:104-110), w = 2 pi softplus(u2):
        a = [-lam u0 - w u1, w u0 - lam u1, u3, -gam^2 u2 - 2 gam u3],   gam = sqrt(3) / ell
        J = [-lam, -w, -w' u1, 0; w, -lam, w' u0, 0; 0, 0, 0, 1; 0, 0, -gam^2, -2 gam]
    Tangents along a direction (d . = the explicit dependence on the direction's constants):
        d a = J dm + (da/dlam) d lam + (da/dgam) d gam
        d J = (dJ/du) [dm] + (dJ/dlam) d lam + (dJ/dgam) d gam
        d (dP/dt) = X + X^T + d Gamma,   X = dJ P + J dP
"""
import numpy as np

TWO_PI = 2.0 * np.pi


def constants(build, theta, Xi, with_dxi=False):
    """The continuous model's constants at g(theta) and their derivatives along every theta_k (and, with_dxi, along Xi as a last
    direction): -> dict of lam, gam, Gamma (4, 4), Xi, m0 (4,), P0 (4, 4) and d<name> with a leading direction axis.
    build: 'chirp' (theta of lam, b, delta, ell, sigma, m0_v) or 'lascala' (delta, ell, sigma, m0_v)."""
    theta = np.asarray(theta, dtype=np.float64)
    with np.errstate(over='ignore'):
        p = np.logaddexp(0.0, theta)                                     # g (models.py:50); theta = -800: 0 exactly
        s = 1.0 / (1.0 + np.exp(-theta))                                 # g'
    n = theta.size
    D = n + (1 if with_dxi else 0)
    if build == 'chirp':
        lam, b, delta, ell, sigma, m0v = p
        i_lam, i_b, i_delta, i_ell, i_sigma, i_m0 = range(6)
    else:
        delta, ell, sigma, m0v = p
        lam = b = 0.0
        i_lam = i_b = None
        i_delta, i_ell, i_sigma, i_m0 = range(4)
    gam = np.sqrt(3.0) / ell
    c = dict(lam=lam, gam=gam, Xi=float(Xi), Gamma=np.diag([b * b, b * b, 0.0, 4.0 * sigma ** 2 * gam ** 3]), m0=np.array([0.0, 0.0, m0v, 0.0]),
             P0=np.diag([delta, delta, sigma ** 2, gam ** 2 * sigma ** 2]))
    dlam, dgam, dXi = np.zeros(D), np.zeros(D), np.zeros(D)
    dG, dm0, dP0 = np.zeros((D, 4, 4)), np.zeros((D, 4)), np.zeros((D, 4, 4))
    if i_lam is not None:
        dlam[i_lam] = s[i_lam]
        dG[i_b, 0, 0] = dG[i_b, 1, 1] = 2.0 * b * s[i_b]
    dgam[i_ell] = -np.sqrt(3.0) / ell ** 2 * s[i_ell]
    dG[i_ell, 3, 3] = 12.0 * sigma ** 2 * gam ** 2 * dgam[i_ell]
    dG[i_sigma, 3, 3] = 8.0 * sigma * gam ** 3 * s[i_sigma]
    dm0[i_m0, 2] = s[i_m0]
    dP0[i_delta, 0, 0] = dP0[i_delta, 1, 1] = s[i_delta]
    dP0[i_sigma, 2, 2] = 2.0 * sigma * s[i_sigma]
    dP0[i_sigma, 3, 3] = 2.0 * sigma * gam ** 2 * s[i_sigma]
    dP0[i_ell, 3, 3] = 2.0 * gam * sigma ** 2 * dgam[i_ell]
    if with_dxi:
        dXi[n] = 1.0
    c.update(dlam=dlam, dgam=dgam, dXi=dXi, dGamma=dG, dm0=dm0, dP0=dP0)
    return c


def _slopes(c, m, P, dm, dP):
    """(a, dP/dt) at (m, P) and their tangents along the directions (dm (D, 4), dP (D, 4, 4))."""
    lam, gam, dlam, dgam = c['lam'], c['gam'], c['dlam'], c['dgam']
    u2 = m[2]
    with np.errstate(over='ignore'):
        sp = np.logaddexp(0.0, u2)
        sg, one_minus = 1.0 / (1.0 + np.exp(-u2)), 1.0 / (1.0 + np.exp(u2))
    w, w1 = TWO_PI * sp, TWO_PI * sg
    w2 = w1 * one_minus
    J = np.array([[-lam, -w, -w1 * m[1], 0.0], [w, -lam, w1 * m[0], 0.0], [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, -gam * gam, -2.0 * gam]])
    a = np.array([-lam * m[0] - w * m[1], w * m[0] - lam * m[1], m[3], -gam * gam * m[2] - 2.0 * gam * m[3]])
    D = dm.shape[0]
    da = dm @ J.T
    da[:, 0] += -dlam * m[0]
    da[:, 1] += -dlam * m[1]
    da[:, 3] += -2.0 * gam * dgam * m[2] - 2.0 * dgam * m[3]
    dJ = np.zeros((D, 4, 4))
    dw = w1 * dm[:, 2]
    dJ[:, 0, 0] = dJ[:, 1, 1] = -dlam
    dJ[:, 0, 1], dJ[:, 1, 0] = -dw, dw
    dJ[:, 0, 2] = -(w2 * dm[:, 2] * m[1] + w1 * dm[:, 1])
    dJ[:, 1, 2] = w2 * dm[:, 2] * m[0] + w1 * dm[:, 0]
    dJ[:, 3, 2] = -2.0 * gam * dgam
    dJ[:, 3, 3] = -2.0 * dgam
    JP = J @ P
    X = dJ @ P + J @ dP
    return a, JP + JP.T + c['Gamma'], da, X + X.transpose(0, 2, 1) + c['dGamma']


def value_and_grad(build, theta, ys, Xi, dt, H=None, with_dxi=False, skip_missing=False):
    """-> (cumulative NLL after every step (T,), its gradient after every step (T, D)); D = theta.size (+ 1: d / d Xi)."""
    c = constants(build, theta, Xi, with_dxi)
    H = np.array([0.0, 1.0, 0.0, 0.0]) if H is None else np.asarray(H, dtype=np.float64)
    m, P, dm, dP = c['m0'].copy(), c['P0'].copy(), c['dm0'].copy(), c['dP0'].copy()
    D = dm.shape[0]
    nll, dnll = 0.0, np.zeros(D)
    nlls, grads = [], []
    for y in np.asarray(ys, dtype=np.float64):
        # ---- RK4 (quadratures.py:49-54) on the state and, beside it, on its tangents
        k1 = _slopes(c, m, P, dm, dP)
        k2 = _slopes(c, *(x + dt * k / 2 for x, k in zip((m, P, dm, dP), k1)))
        k3 = _slopes(c, *(x + dt * k / 2 for x, k in zip((m, P, dm, dP), k2)))
        k4 = _slopes(c, *(x + dt * k for x, k in zip((m, P, dm, dP), k3)))
        m, P, dm, dP = (x + dt * (a + 2 * b + 2 * cc + d) / 6 for x, a, b, cc, d in zip((m, P, dm, dP), k1, k2, k3, k4))
        if not (skip_missing and np.isnan(y)):
            # ---- the update (filters_smoothers.py:55-68) and its tangent
            PH, dPH = P @ H, dP @ H
            S, dS = H @ PH + c['Xi'], dPH @ H + c['dXi']
            K = PH / S
            dK = (dPH - K[None, :] * dS[:, None]) / S
            nu, dnu = y - H @ m, -(dm @ H)
            m, dm = m + K * nu, dm + dK * nu + K[None, :] * dnu[:, None]
            KK = np.outer(K, K)
            dKK = dK[:, :, None] * K[None, None, :] + K[None, :, None] * dK[:, None, :]
            P, dP = P - KK * S, dP - dKK * S - KK[None] * dS[:, None, None]
            nll += 0.5 * (np.log(TWO_PI * S) + nu * nu / S)
            dnll = dnll + 0.5 * (dS / S + 2.0 * nu * dnu / S - nu * nu * dS / (S * S))
        nlls.append(nll)
        grads.append(dnll.copy())
    return np.array(nlls).reshape(-1), np.array(grads).reshape(-1, D)
