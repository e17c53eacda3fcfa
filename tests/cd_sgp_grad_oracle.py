"""The continuous-discrete sigma-point filter's final NLL and its exact gradient in float64 NumPy: a forward-tangent restatement of the
recursion, written from the formulas and not from the kernel (csrc/cgp_tangent4_cd_sigma.hpp) -- dense 4 x 4 matrices, every direction
and every sigma point at once, the derivatives of the model's constants taken analytically (tests/cd_grad_oracle.py: constants; the
kernel's host side takes them by complex step).  tests/test_cd_sgp_gradient_host.py holds it against the 100-digit fixture: float64
reaches the gates before the GPU is asked to.

    cd_sgp_filter (filters_smoothers.py:534-582): per measurement one RK4 step (quadratures.py:34-54) of the sigma-point moment ODE
    (:124-137)
        P = L L^T,   chi_p = m + L xi_p,   dm/dt = sum w_p a(chi_p),   dP/dt = C + C^T + Gamma,   C = sum w_p (chi_p - m) a(chi_p)^T
    then the scalar update (filters_smoothers.py:55-68).  Chirp SDE (models.py:104-110), w = 2 pi softplus(u2):
        a = [-lam u0 - w u1, w u0 - lam u1, u3, -gam^2 u2 - 2 gam u3],   gam = sqrt(3) / ell
    Tangents along a direction (d . = the explicit dependence on the direction's constants):
        dL = L Phi(L^-1 dP L^-T)      Phi: the strict lower triangle and half the diagonal
        d chi_p = dm + dL xi_p        d a_p = J(chi_p) d chi_p + (da/dlam) d lam + (da/dgam) d gam
        d (dm/dt) = sum w_p d a_p     d C = sum w_p (dL xi_p a_p^T + L xi_p d a_p^T)
    ``substeps=n``: n such RK4 steps of dt / n between two measurements.
"""
import numpy as np

from tests.cd_grad_oracle import TWO_PI, constants


def sigma_set(name):
    """The d = 4 sets of the fixture by name -> (xi (s, 4), w (s,)): the library's own SigmaPoints (quadratures.py)."""
    from chirpgp_amd.quadratures import SigmaPoints
    sg = SigmaPoints.cubature(4) if name == 'cubature' else SigmaPoints.gauss_hermite(4, int(name[2:]))
    return np.asarray(sg.xi, dtype=np.float64), np.asarray(sg.w, dtype=np.float64).reshape(-1)


def _phi(A):
    return np.tril(A, -1) + 0.5 * A * np.eye(A.shape[-1])


def _slopes(c, xi, w, m, P, dm, dP):
    """(dm/dt, dP/dt) of the sigma-point moment ODE at (m, P) and their tangents along the directions (dm (D, 4), dP (D, 4, 4))."""
    lam, gam, dlam, dgam = c['lam'], c['gam'], c['dlam'], c['dgam']
    L = np.linalg.cholesky(P)
    Li = np.linalg.inv(L)
    dL = L @ _phi(Li @ dP @ Li.T)                                        # (D, 4, 4)
    lx = xi @ L.T                                                        # (s, 4): L xi_p
    chi = m + lx
    dlx = np.einsum('kij,pj->kpi', dL, xi)                               # (D, s, 4)
    dchi = dm[:, None, :] + dlx
    u2 = chi[:, 2]
    with np.errstate(over='ignore'):
        sp = np.logaddexp(0.0, u2)
        sg = 1.0 / (1.0 + np.exp(-u2))
    om, om1 = TWO_PI * sp, TWO_PI * sg
    a = np.stack([-lam * chi[:, 0] - om * chi[:, 1], om * chi[:, 0] - lam * chi[:, 1], chi[:, 3], -gam * gam * chi[:, 2] - 2.0 * gam * chi[:, 3]], axis=1)
    dom = om1 * dchi[:, :, 2]
    da = np.stack([-dlam[:, None] * chi[:, 0] - dom * chi[:, 1] - lam * dchi[:, :, 0] - om * dchi[:, :, 1],
                   dom * chi[:, 0] - dlam[:, None] * chi[:, 1] + om * dchi[:, :, 0] - lam * dchi[:, :, 1],
                   dchi[:, :, 3],
                   -2.0 * gam * dgam[:, None] * chi[:, 2] - 2.0 * dgam[:, None] * chi[:, 3] - gam * gam * dchi[:, :, 2] - 2.0 * gam * dchi[:, :, 3]], axis=2)
    km = w @ a
    C = np.einsum('p,pi,pj->ij', w, lx, a)
    dkm = np.einsum('p,kpi->ki', w, da)
    dC = np.einsum('p,kpi,pj->kij', w, dlx, a) + np.einsum('p,pi,kpj->kij', w, lx, da)
    return km, C + C.T + c['Gamma'], dkm, dC + dC.transpose(0, 2, 1) + c['dGamma']


def value_and_grad(build, sigma, theta, ys, Xi, dt, H=None, with_dxi=False, skip_missing=False, substeps=1):
    """-> (cumulative NLL after every step (T,), its gradient after every step (T, D)); D = theta.size (+ 1: d / d Xi).  sigma: a name
    of sigma_set or (xi, w).  A covariance without a Cholesky factor gives NaN from there on."""
    c = constants(build, theta, Xi, with_dxi)
    xi, w = sigma_set(sigma) if isinstance(sigma, str) else sigma
    H = np.array([0.0, 1.0, 0.0, 0.0]) if H is None else np.asarray(H, dtype=np.float64)
    m, P, dm, dP = c['m0'].copy(), c['P0'].copy(), c['dm0'].copy(), c['dP0'].copy()
    D = dm.shape[0]
    h = dt / substeps
    nll, dnll = 0.0, np.zeros(D)
    nlls, grads = [], []
    for y in np.asarray(ys, dtype=np.float64):
        try:
            for _ in range(substeps):
                # ---- RK4 (quadratures.py:49-54) on the state and, beside it, on its tangents
                k1 = _slopes(c, xi, w, m, P, dm, dP)
                k2 = _slopes(c, xi, w, *(x + h * k / 2 for x, k in zip((m, P, dm, dP), k1)))
                k3 = _slopes(c, xi, w, *(x + h * k / 2 for x, k in zip((m, P, dm, dP), k2)))
                k4 = _slopes(c, xi, w, *(x + h * k for x, k in zip((m, P, dm, dP), k3)))
                m, P, dm, dP = (x + h * (a + 2 * b + 2 * cc + d) / 6 for x, a, b, cc, d in zip((m, P, dm, dP), k1, k2, k3, k4))
        except np.linalg.LinAlgError:
            nll, dnll = np.nan, np.full(D, np.nan)
            m, P = np.full(4, np.nan), np.full((4, 4), np.nan)
        if not (skip_missing and np.isnan(y)) and np.isfinite(nll):
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
        grads.append(np.array(dnll, dtype=np.float64).copy())
    return np.array(nlls).reshape(-1), np.array(grads).reshape(-1, D)
