"""Writes tests/golden/exact_pcrlb.npz: the posterior Cramer-Rao blocks of hand-placed state pairs in 100-digit arithmetic.

Nothing here knows a Jacobian or a Hessian: the literal Gaussian log-densities log p(x_t | x_s) = log N(x_t; m(x_s), Sigma) and
log p(y | x_t) = log N(y; H . x_t, Xi) are written down in mpmath and differentiated twice numerically (mpmath.diff at 100 digits,
which is good to well beyond float64).  Shares no code with tests/pcrlb_oracle.py or the package.

    python tests/golden/make_exact_pcrlb.py          (about 20 seconds)

Per model `name` the archive holds  name_id / _d / _params / _dt / _H / _Xi / _j0,  the pairs name_xs, name_xt (n, d),
their blocks name_b11, name_b12 (n, d, d):   b11 = -d2 log p / dx_s2,   b12[s][t] = -d/dx_t d/dx_s log p,
name_d22 (d, d) = -d2 log p / dx_t2 - d2 log p(y | x_t) / dx_t2, and a T = 6, N = 5 recursion name_js (6, d, d) whose sample (t, n)
is pair name_rec[t, n]:   J_t = D22 - D12_t^T (J_{t-1} + D11_t)^-1 D12_t with D11_t, D12_t the means over n, J_0 = j0.
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 100
HERE = os.path.dirname(os.path.abspath(__file__))
V_POINTS = (-40.0, -1.75, -1.5, 0.0, 1.5, 2.0, 30.0, 650.0)


def m32(ell, sigma, dt):
    gam = mp.sqrt(3) / ell
    eta = dt * gam
    beta = sigma ** 2 * mp.exp(-2 * eta)
    e = mp.exp(-eta)
    F = mp.matrix([[(1 + eta) * e, dt * e], [-dt * gam ** 2 * e, (1 - eta) * e]])
    off = 2 * dt ** 2 * gam ** 3 * beta
    S = mp.matrix([[sigma ** 2 - beta * (2 * eta + 2 * eta ** 2 + 1), off],
                   [off, gam ** 2 * (sigma ** 2 + beta * (2 * eta - 2 * eta ** 2 - 1))]])
    return F, S


class Harmonic:
    """disc_harmonic_chirp_lcd (models.py:332-386)."""
    model_id = 1

    def __init__(self, lam, b, ell, sigma, fs, nh, dt):
        self.params = [lam, b, ell, sigma, fs]
        self.lam, self.b, self.fs, self.nh, self.dt = (mp.mpf(lam), mp.mpf(b), mp.mpf(fs), nh, mp.mpf(dt))
        self.d = 2 * nh + 2
        self.Fm, Sm = m32(mp.mpf(ell), mp.mpf(sigma), self.dt)
        q = self.b ** 2 / (2 * self.lam) * (1 - mp.exp(-2 * self.lam * self.dt))
        self.Sigma = mp.zeros(self.d)
        for i in range(2 * nh):
            self.Sigma[i, i] = q
        for i in range(2):
            for j in range(2):
                self.Sigma[2 * nh + i, 2 * nh + j] = Sm[i, j]

    def mean(self, u):
        iv = self.d - 2
        w = 2 * mp.pi * mp.log(mp.exp(u[iv]) + 1) * self.fs
        rho = mp.exp(-self.lam * self.dt)
        out = []
        for k in range(1, self.nh + 1):
            c, s = mp.cos(self.dt * k * w) * rho, mp.sin(self.dt * k * w) * rho
            a, b = u[2 * k - 2], u[2 * k - 1]
            out += [c * a - s * b, s * a + c * b]
        out += [self.Fm[0, 0] * u[iv] + self.Fm[0, 1] * u[iv + 1], self.Fm[1, 0] * u[iv] + self.Fm[1, 1] * u[iv + 1]]
        return out


class Linear:
    model_id = 0

    def __init__(self, F, Sigma, dt):
        self.d = F.rows
        self.F, self.Sigma, self.dt = F, Sigma, mp.mpf(dt)
        self.params = [float(F[i, j]) for i in range(self.d) for j in range(self.d)] + \
                      [float(Sigma[i, j]) for i in range(self.d) for j in range(self.d)]

    def mean(self, u):
        return [sum(self.F[i, j] * u[j] for j in range(self.d)) for i in range(self.d)]


def logpdf_transition(model, P, logdet, xt, xs):
    m = model.mean(xs)
    r = [a - b for a, b in zip(xt, m)]
    quad = sum(r[i] * P[i, j] * r[j] for i in range(model.d) for j in range(model.d))
    return -quad / 2 - (model.d * mp.log(2 * mp.pi) + logdet) / 2


def logpdf_likelihood(H, Xi, y, xt):
    e = y - sum(h * x for h, x in zip(H, xt))
    return -e * e / (2 * Xi) - mp.log(2 * mp.pi * Xi) / 2


def second(f, point, i, j):
    """d2 f / dz_i dz_j at `point` (a list of mpf), by mpmath.diff on the one or two coordinates that move."""
    def moved(*z):
        p = list(point)
        p[i] = z[0]
        if j != i:
            p[j] = z[1]
        return f(p)
    if i == j:
        return mp.diff(moved, point[i], 2)
    return mp.diff(moved, (point[i], point[j]), (1, 1))


def blocks(model, P, logdet, xs, xt):
    d = model.d
    f = lambda z: logpdf_transition(model, P, logdet, z[d:], z[:d])          # z = (x_s, x_t)
    z = list(xs) + list(xt)
    b11, b12 = mp.zeros(d), mp.zeros(d)
    for i in range(d):
        for j in range(i + 1):
            b11[i, j] = b11[j, i] = -second(f, z, i, j)
        for t in range(d):
            b12[i, t] = -second(f, z, i, d + t)
    return b11, b12


def d22_of(model, P, logdet, H, Xi, xs, xt):
    d = model.d
    y = mp.mpf('0.37')
    f = lambda z: logpdf_transition(model, P, logdet, z, xs) + logpdf_likelihood(H, Xi, y, z)
    out = mp.zeros(d)
    for i in range(d):
        for j in range(i + 1):
            out[i, j] = out[j, i] = -second(f, list(xt), i, j)
    return out


def to_np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


def pairs_for(model, rng):
    """16 pairs: the frequency state at every point of V_POINTS twice (a linear model has none: 16 draws); pair 3 has r = 0."""
    d = model.d
    sd = [float(mp.sqrt(model.Sigma[i, i])) for i in range(d)]
    xs_all, xt_all = [], []
    for n in range(16):
        u = rng.normal(size=d) * 1.3
        if isinstance(model, Harmonic):
            u[d - 2] = V_POINTS[n % 8]
        m = [float(v) for v in model.mean([mp.mpf(float(v)) for v in u])]
        x = np.array(m) + (0.0 if n == 3 else 1.0) * rng.normal(size=d) * np.array(sd)
        xs_all.append(u)
        xt_all.append(x)
    return np.array(xs_all), np.array(xt_all)


def main():
    rng = np.random.default_rng(20260)
    Fm, Sm = m32(mp.mpf('0.8'), mp.mpf('1.3'), mp.mpf('0.1'))
    models = {
        'chirp': Harmonic(0.5, 0.3, 1.0, 1.0, 1.0, 1, 0.05),
        'nh2': Harmonic(0.4, 0.5, 1.2, 0.9, 0.7, 2, 0.1),
        'nh3': Harmonic(0.7, 0.8, 1.5, 1.1, 0.5, 3, 0.1),
        'm32': Linear(Fm, Sm, 0.1),
    }
    out = {}
    for name, model in models.items():
        d = model.d
        # the matrices of the density at the float64 values the kernels are handed (params), not at their decimal strings
        if isinstance(model, Linear):
            model.F = mp.matrix(d, d)
            model.Sigma = mp.matrix(d, d)
            for i in range(d):
                for j in range(d):
                    model.F[i, j] = mp.mpf(model.params[i * d + j])
                    model.Sigma[i, j] = mp.mpf(model.params[d * d + i * d + j])
        P = model.Sigma ** -1
        logdet = mp.log(mp.det(model.Sigma))
        H = [mp.mpf(1) if (i % 2 == 1 and i < d - 2) or (isinstance(model, Linear) and i == 0) else mp.mpf(0) for i in range(d)]
        Xi = mp.mpf('0.1')
        xs, xt = pairs_for(model, rng)
        b11s, b12s = [], []
        for u, x in zip(xs, xt):
            b11, b12 = blocks(model, P, logdet, [mp.mpf(float(v)) for v in u], [mp.mpf(float(v)) for v in x])
            b11s.append(b11)
            b12s.append(b12)
        D22 = d22_of(model, P, logdet, H, Xi, [mp.mpf(float(v)) for v in xs[0]], [mp.mpf(float(v)) for v in xt[0]])
        rec = np.array([[(5 * t + n) % 16 for n in range(5)] for t in range(6)])
        j0 = np.diag(1.0 / (1.0 + 0.25 * np.arange(d)))
        J = mp.matrix(d, d)
        for i in range(d):
            J[i, i] = mp.mpf(float(j0[i, i]))
        js = []
        for t in range(6):
            D11, D12 = mp.zeros(d), mp.zeros(d)
            for n in rec[t]:
                D11 += b11s[n] / 5
                D12 += b12s[n] / 5
            J = D22 - D12.T * ((J + D11) ** -1 * D12)
            js.append(to_np(J))
        out.update({f'{name}_id': np.int64(model.model_id), f'{name}_d': np.int64(d), f'{name}_params': np.array(model.params, dtype=np.float64),
                    f'{name}_dt': np.float64(float(model.dt)), f'{name}_H': np.array([float(h) for h in H]), f'{name}_Xi': np.float64(float(Xi)),
                    f'{name}_j0': j0, f'{name}_xs': xs, f'{name}_xt': xt,
                    f'{name}_b11': np.array([to_np(b) for b in b11s]), f'{name}_b12': np.array([to_np(b) for b in b12s]),
                    f'{name}_d22': to_np(D22), f'{name}_rec': rec, f'{name}_js': np.array(js)})
        print(name, 'done', flush=True)
    np.savez_compressed(os.path.join(HERE, 'exact_pcrlb.npz'), **out)


if __name__ == '__main__':
    main()
