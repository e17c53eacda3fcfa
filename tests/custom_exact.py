"""The two model families behind tests/golden/exact_custom_*.npz, each written three times from ONE table: as device source for
cgp_model_from_source (csrc/cgp_custom.hpp), as a host callable over NumPy for the oracle, and -- the same Python expression over mpmath --
for the 100-digit generator (tests/golden/make_exact_custom.py).  Shared by tests/test_exact_custom.py (CPU) and tests/test_gpu_custom_exact.py.

1. The operation table: one `measure<T>` body per dimension, a switch over q[0]; q = [operation index, c, s].  Every overload of
   namespace cgp::ad is an operation of its own on u[0], u[1] (or u[0] and the constant c), so that a wrong partial derivative is a wrong H
   of ekf_for_kpt's update and a wrong value a wrong innovation.
2. The ring: drift a_i = -p0 u_i + p1 sin(u_{i+1}) + p2 u_i u_{i-1} (indices mod DIM), discrete mean u + dt a(u), discrete covariance
   dt (p3 I + v v^T) with v_i = p4 cos(u_i) -- state-dependent and dense -- written once for every DIM = 1..8."""
import numpy as np


class NP:
    """the elementary functions over float64 / complex128 (the oracle differentiates by the complex step)"""
    sin, cos, exp, log, sqrt, tanh = np.sin, np.cos, np.exp, np.log, np.sqrt, np.tanh

    @staticmethod
    def softplus(x):
        return np.log(np.exp(x) + 1)                        # models.py:50, the naive form, as cgp::ad::softplus


DD, DC, CD = '(Dual,Dual)', '(Dual,double)', '(double,Dual)'
CHAIN = 'chain(Dual,double,double)'
# (name, gate group, needs positive operands, host expression f(M, u, c, s, n), device statement, the declarations of namespace ad it runs);
# n = the dimension: the deep composition reads u[2] and u[3 % n]
OPS = (
    ('add_dd', 'arith', False, lambda M, u, c, s, n: u[0] + u[1], 'return u[0] + u[1];', ('operator+' + DD,)),
    ('sub_dd', 'arith', False, lambda M, u, c, s, n: u[0] - u[1], 'return u[0] - u[1];', ('operator-' + DD,)),
    ('mul_dd', 'arith', False, lambda M, u, c, s, n: u[0] * u[1], 'return u[0] * u[1];', ('operator*' + DD,)),
    ('div_dd', 'arith', False, lambda M, u, c, s, n: u[0] / u[1], 'return u[0] / u[1];', ('operator/' + DD,)),
    ('add_dc', 'arith', False, lambda M, u, c, s, n: u[0] + c, 'return u[0] + c;', ('operator+' + DC,)),
    ('add_cd', 'arith', False, lambda M, u, c, s, n: c + u[0], 'return c + u[0];', ('operator+' + CD,)),
    ('sub_dc', 'arith', False, lambda M, u, c, s, n: u[0] - c, 'return u[0] - c;', ('operator-' + DC,)),
    ('sub_cd', 'arith', False, lambda M, u, c, s, n: c - u[0], 'return c - u[0];', ('operator-' + CD,)),
    ('mul_dc', 'arith', False, lambda M, u, c, s, n: u[0] * c, 'return u[0] * c;', ('operator*' + DC,)),
    ('mul_cd', 'arith', False, lambda M, u, c, s, n: c * u[0], 'return c * u[0];', ('operator*' + CD,)),
    ('div_dc', 'arith', False, lambda M, u, c, s, n: u[0] / c, 'return u[0] / c;', ('operator/' + DC,)),
    ('div_cd', 'arith', False, lambda M, u, c, s, n: c / u[0], 'return c / u[0];', ('operator/' + CD,)),
    ('neg', 'arith', False, lambda M, u, c, s, n: -u[0], 'return -u[0];', ('operator-(Dual)',)),
    ('iadd_d', 'arith', False, lambda M, u, c, s, n: u[0] + u[1], '{ T a = u[0]; a += u[1]; return a; }', ('operator+=' + DD,)),
    ('isub_d', 'arith', False, lambda M, u, c, s, n: u[0] - u[1], '{ T a = u[0]; a -= u[1]; return a; }', ('operator-=' + DD,)),
    ('imul_d', 'arith', False, lambda M, u, c, s, n: u[0] * u[1], '{ T a = u[0]; a *= u[1]; return a; }', ('operator*=' + DD,)),
    ('iadd_c', 'arith', False, lambda M, u, c, s, n: u[0] + c, '{ T a = u[0]; a += c; return a; }', ('operator+=' + DC,)),
    ('imul_c', 'arith', False, lambda M, u, c, s, n: u[0] * c, '{ T a = u[0]; a *= c; return a; }', ('operator*=' + DC,)),
    ('imul_self', 'arith', False, lambda M, u, c, s, n: u[0] * u[0], '{ T a = u[0]; a *= a; return a; }', ('operator*=' + DD,)),
    ('iadd_self', 'arith', False, lambda M, u, c, s, n: u[0] + u[0], '{ T a = u[0]; a += a; return a; }', ('operator+=' + DD,)),
    ('construct', 'arith', False, lambda M, u, c, s, n: c * u[0] + c, '{ T k(c); return k * u[0] + k; }', ('Dual(double)',)),
    ('lit_mul', 'arith', False, lambda M, u, c, s, n: 2 * u[0], 'return 2 * u[0];', ('operator*' + CD,)),
    ('lit_div', 'arith', False, lambda M, u, c, s, n: u[0] / 3, 'return u[0] / 3;', ('operator/' + DC,)),
    ('lit_rdiv', 'arith', False, lambda M, u, c, s, n: 1 / u[0], 'return 1 / u[0];', ('operator/' + CD,)),
    # a denominator of value 1e-150 (s): its reciprocal is 1e150 and nothing on the way may be squared; brought back to O(1) by * s
    ('div_cd_tiny', 'arith', False, lambda M, u, c, s, n: (c / (u[0] * s)) * s, 'return (c / (u[0] * s)) * s;', ('operator/' + CD,)),
    ('div_dd_tiny', 'arith', False, lambda M, u, c, s, n: (u[1] / (u[0] * s)) * s, 'return (u[1] / (u[0] * s)) * s;', ('operator/' + DD,)),
    ('softplus_c', 'arith', False, lambda M, u, c, s, n: u[0] * M.softplus(c), 'return u[0] * softplus(c);', ('softplus(double)',)),
    ('sin', 'func', False, lambda M, u, c, s, n: M.sin(u[0]), 'return sin(u[0]);', ('sin(Dual)', CHAIN)),
    ('cos', 'func', False, lambda M, u, c, s, n: M.cos(u[0]), 'return cos(u[0]);', ('cos(Dual)', CHAIN)),
    ('exp', 'func', False, lambda M, u, c, s, n: M.exp(u[0]), 'return exp(u[0]);', ('exp(Dual)', CHAIN)),
    ('log', 'func', True, lambda M, u, c, s, n: M.log(u[0]), 'return log(u[0]);', ('log(Dual)', CHAIN)),
    ('sqrt', 'func', True, lambda M, u, c, s, n: M.sqrt(u[0]), 'return sqrt(u[0]);', ('sqrt(Dual)', CHAIN)),
    ('tanh', 'func', False, lambda M, u, c, s, n: M.tanh(u[0]), 'return tanh(u[0]);', ('tanh(Dual)', CHAIN)),
    ('softplus', 'func', False, lambda M, u, c, s, n: M.softplus(u[0]), 'return softplus(u[0]);', ('softplus(Dual)', CHAIN)),
    # sqrt at 1e-200 (s): the derivative 0.5 / 1e-100; brought back to O(1) by / c with c = 1e-100
    ('sqrt_tiny', 'func', True, lambda M, u, c, s, n: M.sqrt(u[0] * s) / c, 'return sqrt(u[0] * s) / c;', ('sqrt(Dual)', CHAIN)),
    ('pow', 'pow', True, lambda M, u, c, s, n: u[0] ** c + u[1], 'return pow(u[0], c) + u[1];', ('pow(Dual,double)', CHAIN)),
    ('deep', 'comp', True, lambda M, u, c, s, n: M.sin(M.exp(c * u[0]) * u[1]) / M.sqrt(u[2] * u[2] + 1) + M.tanh(u[3 % n]) * M.log(u[0] + 2),
     'return sin(exp(c * u[0]) * u[1]) / sqrt(u[2] * u[2] + 1) + tanh(u[3 % DIM]) * log(u[0] + 2);', ()),
    ('bump', 'comp', True, lambda M, u, c, s, n: M.exp(-u[0] * u[0]) * M.tanh(u[1] * c) + M.sqrt(M.softplus(u[0] + u[1])),
     'return exp(-u[0] * u[0]) * tanh(u[1] * c) + sqrt(softplus(u[0] + u[1]));', ()),
    ('logistic', 'comp', False, lambda M, u, c, s, n: (M.cos(u[0]) * M.cos(u[0]) + 1.5) ** c / (1.0 + M.exp(-u[1])),
     'return pow(cos(u[0]) * cos(u[0]) + 1.5, c) / (1.0 + exp(-u[1]));', ()),
    ('assign', 'comp', False, lambda M, u, c, s, n: _assign(M, u, c),
     '{ T a = sin(u[0]); a *= u[1]; a += c; a -= cos(a); return a / (2.0 + a * a); }', ()),
)
OP_INDEX = {op[0]: i for i, op in enumerate(OPS)}
GROUPS = ('arith', 'func', 'pow', 'comp')


def _assign(M, u, c):
    a = M.sin(u[0]) * u[1] + c
    a = a - M.cos(a)
    return a / (2.0 + a * a)


def ops_source(d):
    """the measurement body of the whole table at dimension d: one compilation, the operation chosen per trial"""
    cases = '\n'.join(f'    case {i}: {op[4]}' for i, op in enumerate(OPS))
    return (f'constexpr int DIM = {d};\n'
            'template <class T> __device__ T measure(const T* u, const double* q) {\n'
            '    const double c = q[1], s = q[2];\n'
            '    switch ((int)q[0]) {\n' + cases + '\n    }\n    return T(0.0);\n}\n')


def ops_host(q, d, M=NP):
    """h(u) of one trial: q = [operation index, c, s] as Python floats (exact in either arithmetic)"""
    f, c, s = OPS[int(q[0])][3], float(q[1]), float(q[2])
    return lambda u: f(M, u, c, s, d)


RING = r'''
template <class T> __device__ void drift(const T* u, const double* p, T* a) {
#pragma unroll
    for (int i = 0; i < DIM; i++) a[i] = -p[0] * u[i] + p[1] * sin(u[(i + 1) % DIM]) + p[2] * u[i] * u[(i + DIM - 1) % DIM];
}
template <class T> __device__ void cond_mean(const T* u, const double* p, double dt, T* m) {
    T a[DIM];
    drift(u, p, a);
#pragma unroll
    for (int i = 0; i < DIM; i++) m[i] = u[i] + dt * a[i];
}
__device__ void cond_cov(const double* u, const double* p, double dt, double* cov) {
    double v[DIM];
    for (int i = 0; i < DIM; i++) v[i] = p[4] * cos(u[i]);
    for (int i = 0; i < DIM; i++)
        for (int j = 0; j < DIM; j++) cov[i * DIM + j] = dt * ((i == j ? p[3] : 0.0) + v[i] * v[j]);
}
'''


def ring_source(d):
    return f'constexpr int DIM = {d};' + RING


def ring_host(p, M=NP, lists=False):
    """(drift(u), cond_m_cov(u, dt)) of the ring with parameter row p; lists=True: plain lists (the mpmath generator), else arrays"""
    p = [float(v) for v in p]

    def drift(u):
        n = len(u)
        a = [-p[0] * u[i] + p[1] * M.sin(u[(i + 1) % n]) + p[2] * u[i] * u[(i + n - 1) % n] for i in range(n)]
        return a if lists else np.array(a)

    def cond_m_cov(u, dt):
        n = len(u)
        a = drift(u)
        v = [p[4] * M.cos(u[i]) for i in range(n)]
        mean = [u[i] + dt * a[i] for i in range(n)]
        cov = [[dt * ((p[3] if i == j else 0.0) + v[i] * v[j]) for j in range(n)] for i in range(n)]
        return (mean, cov) if lists else (np.array(mean), np.real(np.array(cov)))
    return drift, cond_m_cov


METHODS = ('ekf', 'eks', 'sgp_filter', 'sgp_smoother', 'cd_ekf', 'cd_eks', 'cd_sgp_filter', 'cd_sgp_smoother')
SIGMA_METHODS = METHODS[2:4] + METHODS[6:]
