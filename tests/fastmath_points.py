"""What the tests of the in-kernel elementary functions (chirpgp_amd/csrc/cgp_fastmath.hpp) share: the header's coefficient tables and
constants read out of its text, each polynomial's error measured in 200-bit arithmetic (test_fastmath_tables.py asserts them against
what the header prints; test_gpu_fastmath_edges.py takes them as the inputs of its per-point gates), and the deterministic generators
of the points where these functions can break: the ends of the range reductions, the high-word thresholds that switch regime, the
ends of the mantissa interval, subnormal results."""
import functools
import os
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'chirpgp_amd', 'csrc', 'cgp_fastmath.hpp')
PREC = 200
GRID = 4001                                     # points per interval, ends included
# the scales cgp_debug_math folds into the coefficients of ops 14 / 15 (cgp_api.hip: kDebugScale, kDebugDscale)
DEBUG_SCALE, DEBUG_DSCALE = 0.0439822971502571, 2.7

_NUM = r'[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?'


@functools.lru_cache(maxsize=None)
def header_text(path=HEADER):
    with open(path) as f:
        return f.read()


def _entry(tok):
    """A table entry as the compiler evaluates it: a literal, or the correctly rounded quotient of two literals."""
    tok = tok.strip()
    m = re.fullmatch(rf'({_NUM})\s*/\s*({_NUM})', tok)
    if m:
        return float(m.group(1)) / float(m.group(2))
    if not re.fullmatch(_NUM, tok):
        raise ValueError(f'table entry {tok!r} is neither a literal nor a quotient of two')
    return float(tok)


@functools.lru_cache(maxsize=None)
def tables(path=HEADER):
    """{name: [float, ...]} of every `constexpr double k...[N] = {...}` of the header, in the order written."""
    out = {}
    for m in re.finditer(r'constexpr\s+double\s+(k\w+)\s*\[\s*(\d+)\s*\]\s*=\s*\{([^}]*)\}', header_text(path)):
        body = re.sub(r'//[^\n]*', '', m.group(3))
        vals = [_entry(t) for t in body.split(',') if t.strip()]
        assert len(vals) == int(m.group(2)), (m.group(1), len(vals))
        out[m.group(1)] = vals
    return out


@functools.lru_cache(maxsize=None)
def scalars(path=HEADER):
    """{name: float} of every `constexpr double k... = literal;` of the header."""
    return {m.group(1): float(m.group(2)) for m in re.finditer(rf'constexpr\s+double\s+(k\w+)\s*=\s*({_NUM})\s*;', header_text(path))}


def high_word(x):
    return struct.unpack('<Q', struct.pack('<d', float(x)))[0] >> 32


def low_word(x):
    return struct.unpack('<Q', struct.pack('<d', float(x)))[0] & 0xFFFFFFFF


def from_words(hi, lo):
    return struct.unpack('<d', struct.pack('<Q', (int(hi) << 32) | int(lo)))[0]


@functools.lru_cache(maxsize=None)
def thresholds(path=HEADER):
    """Every 32-bit hexadecimal constant of the header that is the high word of a positive normal double at or above 1, by pattern (sign
    and NaN masks such as 0x7fffffff fall outside): {high word: the double whose low word is zero}."""
    words = {int(w, 16) for w in re.findall(r'0[xX]([0-9A-Fa-f]{8})[uU]?\b', header_text(path))}
    return {w: from_words(w, 0) for w in sorted(words) if 0x3FF00000 <= w < 0x7FF00000}


# ---- the polynomials in 200-bit arithmetic ---------------------------------------------------------------------------------------
def _poly_low_first(c, x):
    import mpmath as mp
    p = mp.mpf(0)
    for v in reversed(c):
        p = p * x + mp.mpf(v)
    return p


def _grid(a, b, n=GRID):
    import mpmath as mp
    a, b = mp.mpf(a), mp.mpf(b)
    return [a + (b - a) * k / (n - 1) for k in range(n - 1)] + [b]


def _max_err(approx, exact, a, b, relative):
    worst = 0
    for x in _grid(a, b):
        w = exact(x)
        e = abs(approx(x) - w)
        if relative:
            e = e / abs(w)
        worst = max(worst, e)
    return float(worst)


# What the header prints for each approximation (its comment's figure, which must also be found in the header's text).
PRINTED = {'exp_lean': '5.5e-11', 'q_lean': '1.0e-11', 'exp_high': '2.5e-9', 'q_high': '2.4e-9', 'sig_high': '2.7e-14',
           'mid_g': '2.5e-16', 'mid_h': '4.3e-16'}
# ... and for the truncation of each series
TRUNCATION = {'exp_taylor': '5.2e-18', 'sin_taylor': '5e-17', 'cos_taylor': '5e-17', 'atanh': '2e-17', 'log1p_series': '1e-19'}


def holds(measured, printed):
    """measured <= printed + half a unit of printed's last digit"""
    mant, exp = printed.lower().split('e')
    decimals = len(mant.split('.')[1]) if '.' in mant else 0
    return measured <= float(printed) + 0.5 * 10.0 ** (int(exp) - decimals)


def _jobs(path):
    import mpmath as mp
    T = tables(path)
    ln2h = mp.log(2) / 2
    q = lambda t: mp.log1p(t) / t if t != 0 else mp.mpf(1)
    g = lambda w: mp.log(2 * mp.cosh(mp.sqrt(w) / 2))
    h = lambda w: mp.tanh(mp.sqrt(w) / 2) / (2 * mp.sqrt(w)) if w != 0 else mp.mpf(1) / 4
    low = lambda name: (lambda x: _poly_low_first(T[name], x))
    high = lambda name: (lambda x: _poly_low_first(T[name][::-1], x))

    # sin r = r - r^3 ps(r^2), cos r = 1 - r^2 / 2 + r^4 pc(r^2), the tables highest power first
    def sin_series(r):
        return r - r ** 3 * _poly_low_first(T['kSinTaylor'][::-1], r * r)

    def cos_series(r):
        return 1 - r * r / 2 + r ** 4 * _poly_low_first(T['kCosTaylor'][::-1], r * r)

    # log m = 2 s (1 + s^2 (1/3 + s^2 / 5 + ...)), s = (m - 1) / (m + 1), |s| <= 0.1716: relative to log m = 2 atanh s
    def atanh_ratio(s):
        return 2 * s * (1 + s * s * _poly_low_first(T['kAtanhOdd'][::-1], s * s)) / (2 * mp.atanh(s)) if s != 0 else mp.mpf(1)

    return {
        'exp_lean': lambda: _max_err(low('kExpLean'), mp.exp, -ln2h, ln2h, True),
        'q_lean': lambda: _max_err(low('kLog1pOverTLean'), q, 0, mp.exp(mp.mpf('-1.5')), True),
        'exp_high': lambda: _max_err(low('kExpHigh'), mp.exp, -ln2h, ln2h, True),
        'q_high': lambda: _max_err(low('kLog1pOverTHigh'), q, 0, mp.exp(-5), True),
        'sig_high': lambda: _max_err(low('kSigmoidHigh'), lambda t: 1 / (1 + t), 0, mp.exp(-5), True),
        'mid_g': lambda: _max_err(low('kSoftplusMidG'), g, 0, mp.mpf('4.0008'), True),
        'mid_h': lambda: _max_err(low('kSoftplusMidH'), h, 0, mp.mpf('4.0008'), True),
        'exp_taylor': lambda: _max_err(high('kExpTaylor'), mp.exp, -ln2h, ln2h, True),
        'sin_taylor': lambda: _max_err(sin_series, mp.sin, -mp.pi / 4, mp.pi / 4, False),
        'cos_taylor': lambda: _max_err(cos_series, mp.cos, -mp.pi / 4, mp.pi / 4, False),
        'atanh': lambda: _max_err(atanh_ratio, lambda s: mp.mpf(1), mp.mpf('-0.1716'), mp.mpf('0.1716'), False),
        'log1p_series': lambda: _max_err(lambda t: t * _poly_low_first(T['kLog1pSeries'][::-1], t), mp.log1p, 0, mp.mpf('2.5e-3'), False),
    }


@functools.lru_cache(maxsize=None)
def measure(key, path=HEADER):
    """The error of one polynomial of the header on its interval, GRID points, 200 bits; key: of PRINTED or TRUNCATION.  Relative errors,
    except the sin / cos series and log1p's (absolute, as the header states them)."""
    import mpmath as mp
    with mp.workprec(PREC):
        return _jobs(path)[key]()


def measured(path=HEADER):
    return {key: measure(key, path) for key in list(PRINTED) + list(TRUNCATION)}


def cheb_fit(f, a, b, deg, prec=300):
    """tools/gen_math_constants.py's recipe: the interpolant of f at the Chebyshev nodes of [a, b], coefficients (lowest first) rounded
    to float64."""
    import mpmath as mp
    with mp.workprec(prec):
        a, b = a(), b()
        n = deg + 1
        xs = [(a + b) / 2 + (b - a) / 2 * mp.cos(mp.pi * (2 * k + 1) / (2 * n)) for k in range(n)]
        V = mp.matrix(n, n)
        for i, x in enumerate(xs):
            for j in range(n):
                V[i, j] = x ** j
        c = mp.lu_solve(V, mp.matrix([f(x) for x in xs]))
        return [float(c[j]) for j in range(n)]


# ---- generators ------------------------------------------------------------------------------------------------------------------
def nudge(x, n):
    """x moved by n units in the last place (n < 0: towards -inf)"""
    x = np.array(x, dtype=np.float64)
    for _ in range(abs(int(n))):
        x = np.nextafter(x, np.inf if n > 0 else -np.inf)
    return x


def _rint(v):
    return np.rint(v)                           # round half to even, as v_rndne_f64


@functools.lru_cache(maxsize=None)
def exp_boundary_points():
    """(x, k): the doubles nearest (k + 1/2) ln 2 and their +-1, +-2 ulp neighbours, k = -1075 .. 1024 -- the ends of exp's range
    reduction, where k = rint(x log2 e) goes either way and |r| is at its largest."""
    import mpmath as mp
    with mp.workprec(PREC):
        ln2 = mp.log(2)
        ks = np.arange(-1075, 1025)
        centre = np.array([float((int(k) + mp.mpf(1) / 2) * ln2) for k in ks])
    x = np.concatenate([nudge(centre, n) for n in (-2, -1, 0, 1, 2)])
    return x, np.tile(ks, 5)


def exp_edge_points():
    """... with +-1 ulp around the overflow and underflow selects of fast_exp, and all of (-745.2, -708.4), where results are subnormal."""
    x, _ = exp_boundary_points()
    sel = np.concatenate([nudge(709.782712893384, n) for n in (-1, 0, 1)] + [nudge(-745.2, n) for n in (-1, 0, 1)], axis=None)
    sub = np.linspace(-745.2, -708.4, 302)[1:-1]
    return np.concatenate([x, sel, sub])


def log_points(below_one):
    """fast_log_ge1's hard points: the ends of the mantissa interval 2^k sqrt(2), 2^k sqrt(1/2), each + 0 .. 3 and - 0 .. 3 ulp, the powers of two, 1 +
    1 .. 4 ulp, the largest double; below_one: the same over all positive normals, 1 - 1 .. 4 ulp, (0, 1) log-uniform down to the smallest
    normal, and u = 2^-53 (odd integer) as cgp_rng.hpp forms its uniforms."""
    S = scalars()
    k = np.arange(-1022 if below_one else 0, 1024)
    ends = []
    for root in (S['kSqrt2'], S['kSqrtHalf']):
        base = np.ldexp(root, k + (1 if root < 1 else 0))
        base = base[np.isfinite(base)]
        ends += [nudge(base, n) for n in range(-3, 4)]
    pts = ends + [np.ldexp(1.0, k), nudge(1.0, 1), nudge(1.0, 2), nudge(1.0, 3), nudge(1.0, 4), [1.0, np.finfo(np.float64).max]]
    if below_one:
        rng = np.random.default_rng(101)
        tiny = np.finfo(np.float64).tiny
        odd = 2 * rng.integers(0, 2 ** 52, 2000, dtype=np.int64) + 1
        odd = np.concatenate([odd, [1, 3, 2 ** 53 - 1, 2 ** 53 - 3, 2 ** 52 + 1, 2 ** 52 - 1]])
        pts += [nudge(1.0, -1), nudge(1.0, -2), nudge(1.0, -3), nudge(1.0, -4), [tiny, nudge(tiny, 1)],
                np.exp(rng.uniform(np.log(tiny), 0.0, 2000)), np.ldexp(odd.astype(np.float64), -53)]
    z = np.unique(np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.float64)) for p in pts]))
    lo = np.finfo(np.float64).tiny if below_one else 1.0
    return z[(z >= lo) & np.isfinite(z)]


@functools.lru_cache(maxsize=None)
def pio2_points():
    """(x, n): the double nearest n pi/2 for every n with n pi/2 < 1e5 -- where the reduced argument is at its smallest (6e-19 at n = 29 2^j) and
    the Cody-Waite reduction has the most to cancel."""
    import mpmath as mp
    with mp.workprec(300):
        h = mp.pi / 2
        n = np.arange(1, 63662)
        x = np.array([float(int(i) * h) for i in n])
    return x, n


def sincos_edge_points():
    """the two doubles either side of 1e5 (the last of the fast path, the first of the library's) and one with 1e5's high word and low bits set"""
    hw = high_word(1.0e5)
    return np.array([nudge(1.0e5, -1), 1.0e5, nudge(1.0e5, 1), from_words(hw, 0x9ABCDEF1)], dtype=np.float64)


def threshold_points(values, negatives=False):
    """Per threshold: the threshold itself, the next double below, and one value with the threshold's high word and a non-zero low word."""
    pts = []
    for v in values:
        pts += [float(v), float(nudge(v, -1)), from_words(high_word(v), 0x9ABCDEF1)]
    pts = np.array(pts, dtype=np.float64)
    return np.concatenate([pts, -pts]) if negatives else pts


def exp_reduction_k(x):
    """k = rint(x log2 e) as exp_reduce forms it in float64"""
    return _rint(np.asarray(x, dtype=np.float64) * scalars()['kLog2e'])


def pio2_reduction_n(x):
    return _rint(np.asarray(x, dtype=np.float64) * scalars()['kTwoOverPi'])
