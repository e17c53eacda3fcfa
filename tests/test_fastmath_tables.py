"""The coefficient tables and constants of csrc/cgp_fastmath.hpp, read out of the header's text and checked on the CPU in 200-bit
arithmetic: every approximation error and truncation figure the header prints, the entries that are exact by construction, the split
reduction constants, the high-word thresholds that switch regime -- and the claims of the point generators that the GPU edge tests
(test_gpu_fastmath_edges.py) rely on."""
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

from tests import fastmath_points as fp


def _bits(x):
    """significant bits of a double"""
    n = abs(Fraction(float(x)).numerator)
    return n.bit_length() - ((n & -n).bit_length() - 1) if n else 0


def _rounded(v):
    with mp.workprec(fp.PREC):
        return float(v())


@pytest.mark.parametrize('key', sorted(fp.PRINTED))
def test_approximation_error_the_header_prints(key):
    """Each polynomial on its interval, 4001 points with the ends, against the function at 200 bits: within half a unit of the last printed digit."""
    got = fp.measure(key)
    print(f'{key}: measured {got:.3e}, the header prints {fp.PRINTED[key]}')
    assert fp.PRINTED[key] in fp.header_text(), 'the figure is no longer what the header prints'
    assert fp.holds(got, fp.PRINTED[key]), (key, got)


@pytest.mark.parametrize('key', sorted(fp.TRUNCATION))
def test_truncation_figure_the_header_prints(key):
    got = fp.measure(key)
    print(f'{key}: measured {got:.3e}, the header prints {fp.TRUNCATION[key]}')
    assert fp.TRUNCATION[key] in fp.header_text(), 'the figure is no longer what the header prints'
    assert fp.holds(got, fp.TRUNCATION[key]), (key, got)


def test_fitted_tables_are_what_the_recipe_gives():
    """tools/gen_math_constants.py's recipe (interpolation at the Chebyshev nodes, solved at 300 / 400 bits, rounded to float64) gives
    every fitted table back to the last digit: a digit changed anywhere, also one too small to move an error figure, shows here."""
    T = fp.tables()
    zero = lambda: mp.mpf(0)
    ln2h = lambda sign: (lambda: sign * mp.log(2) / 2 * mp.mpf('1.0001'))
    q = lambda t: mp.log1p(t) / t if t != 0 else mp.mpf(1)
    g = lambda w: mp.log(2 * mp.cosh(mp.sqrt(w) / 2)) if w > 0 else mp.log(2)
    h = lambda w: mp.tanh(mp.sqrt(w) / 2) / (2 * mp.sqrt(w)) if w > 0 else mp.mpf(1) / 4
    wmax = lambda: mp.mpf(4) * mp.mpf('1.0002')
    assert fp.cheb_fit(mp.exp, ln2h(-1), ln2h(1), 7) == T['kExpLean']
    assert fp.cheb_fit(q, zero, lambda: mp.exp(mp.mpf('-1.5')), 7) == T['kLog1pOverTLean']
    assert fp.cheb_fit(mp.exp, ln2h(-1), ln2h(1), 6) == T['kExpHigh']
    assert fp.cheb_fit(q, zero, lambda: mp.exp(mp.mpf(-5)), 2) == T['kLog1pOverTHigh']
    assert fp.cheb_fit(lambda t: 1 / (1 + t), zero, lambda: mp.exp(mp.mpf(-5)), 4) == T['kSigmoidHigh']
    assert fp.cheb_fit(g, zero, wmax, 14, prec=400) == T['kSoftplusMidG']
    assert fp.cheb_fit(h, zero, wmax, 14, prec=400) == T['kSoftplusMidH']


def test_series_tables_are_the_correctly_rounded_exact_values():
    T = fp.tables()
    with mp.workprec(fp.PREC):
        assert T['kExpTaylor'] == [float(1 / mp.factorial(13 - i)) for i in range(14)]
        assert T['kAtanhOdd'] == [float(mp.mpf(1) / (21 - 2 * i)) for i in range(10)]
        assert T['kLog1pSeries'] == [float(mp.mpf((-1) ** (n + 1)) / n) for n in range(6, 0, -1)]
        # sin r = r - r^3 (1/3! - r^2/5! + ...): the coefficient of 1 / (2 j + 1)! carries (-1)^(j + 1);  cos r = 1 - r^2/2 + r^4 (1/4! - r^2/6! + ...): (-1)^j
        assert T['kSinTaylor'] == [float(mp.mpf((-1) ** (j + 1)) / mp.factorial(2 * j + 1)) for j in range(8, 0, -1)]
        assert T['kCosTaylor'] == [float(mp.mpf((-1) ** j) / mp.factorial(2 * j)) for j in range(8, 1, -1)]
    assert set(T) == {'kExpTaylor', 'kExpLean', 'kLog1pOverTLean', 'kExpHigh', 'kLog1pOverTHigh', 'kSigmoidHigh', 'kAtanhOdd', 'kLog1pSeries',
                      'kSinTaylor', 'kCosTaylor', 'kSoftplusMidG', 'kSoftplusMidH'}, 'a table this file does not check'


def test_reduction_constants():
    S = fp.scalars()
    assert _bits(S['kLn2Hi']) <= 32 and _bits(S['kPio2_1']) <= 33 and _bits(S['kPio2_2']) <= 33
    # the last part of each split is the correctly rounded remainder: the sum agrees with the constant to the bits the parts can hold
    assert S['kLn2Lo'] == _rounded(lambda: mp.log(2) - mp.mpf(S['kLn2Hi']))
    assert S['kPio2_3'] == _rounded(lambda: mp.pi / 2 - mp.mpf(S['kPio2_1']) - mp.mpf(S['kPio2_2']))
    # ... and the leading parts are the constant rounded to their bits: what is left is below half a unit of the part's last bit
    with mp.workprec(fp.PREC):
        assert abs(mp.log(2) - mp.mpf(S['kLn2Hi'])) <= mp.ldexp(1, -1 - 32 - 1)                 # ln 2 in [1/2, 1): bit 32 is 2^-33
        assert abs(mp.pi / 2 - mp.mpf(S['kPio2_1'])) <= mp.ldexp(1, 0 - 33)                      # pi/2 in [1, 2): bit 33 is 2^-32
        rest = mp.pi / 2 - mp.mpf(S['kPio2_1'])
        assert abs(rest - mp.mpf(S['kPio2_2'])) <= mp.ldexp(1, int(mp.floor(mp.log(abs(rest), 2))) - 33)
    # the one-constant reduction's ln 2 (SpecRegs: kLn2Hi + kLn2Lo in float64) is ln 2 correctly rounded
    assert S['kLn2Hi'] + S['kLn2Lo'] == _rounded(lambda: mp.log(2))
    assert S['kLog2e'] == _rounded(lambda: 1 / mp.log(2))
    assert S['kTwoOverPi'] == _rounded(lambda: 2 / mp.pi)
    assert S['kSqrtHalf'] == _rounded(lambda: mp.sqrt(mp.mpf(1) / 2))
    assert S['kSqrt2'] == _rounded(lambda: mp.sqrt(2))
    assert S['kPiOver4'] == _rounded(lambda: mp.pi / 4)
    assert set(S) == {'kLog2e', 'kLn2Hi', 'kLn2Lo', 'kTwoOverPi', 'kPio2_1', 'kPio2_2', 'kPio2_3', 'kSqrtHalf', 'kSqrt2', 'kPiOver4'}, \
        'a constant this file does not check'


def test_high_word_thresholds():
    """Collected by pattern, so that a new one is not missed: each is the high word of exactly the double its comment names."""
    thr = fp.thresholds()
    assert sorted(thr.values()) == [1.5, 6.0, 40.0, 700.0, 1.0e5], {hex(k): v for k, v in thr.items()}
    for word, value in thr.items():
        assert fp.high_word(value) == word and fp.low_word(value) == 0
    assert fp.high_word(1.0e5) == 0x40F86A00 and fp.low_word(1.0e5) == 0
    # the literal overflow / underflow selects of fast_exp are written as decimal doubles
    for lit in ('709.782712893384', '-745.2', '700.0', '1.0e5', '1.5'):
        assert lit in fp.header_text()


def test_a_wrong_digit_is_seen(tmp_path):
    """The checks above on a copy of the header with one digit of kExpHigh[3] changed: the error figure moves past what the header prints."""
    text = fp.header_text()
    assert text.count('0.16666415414041177') == 1
    bad = tmp_path / 'cgp_fastmath.hpp'
    bad.write_text(text.replace('0.16666415414041177', '0.16666425414041177'))
    assert fp.tables(str(bad))['kExpHigh'][3] != fp.tables()['kExpHigh'][3]
    assert not fp.holds(fp.measure('exp_high', str(bad)), fp.PRINTED['exp_high'])


# ---- the generators' claims --------------------------------------------------------------------------------------------------------
def test_exp_boundary_points_sit_at_the_ends_of_the_reduction():
    """Each point reduces with |r| within 3 ulp (of the point) of ln 2 / 2, with the k of its own side of the boundary."""
    x, k = fp.exp_boundary_points()
    assert x.size == 5 * 2100
    kk = fp.exp_reduction_k(x)
    assert np.all((kk == k) | (kk == k + 1))
    assert np.any(kk == k) and np.any(kk == k + 1)
    ulp = np.spacing(np.abs(x))
    with mp.workprec(fp.PREC):
        ln2 = mp.log(2)
        for xi, ki, ui in zip(x, kk, ulp):
            r = mp.mpf(float(xi)) - int(ki) * ln2
            assert abs(abs(r) - ln2 / 2) <= 3 * mp.mpf(float(ui)), (xi, ki)
    edge = fp.exp_edge_points()
    assert np.sum((edge > -745.2) & (edge < -708.4)) >= 300 and edge.min() < -745.2 and edge.max() > 709.782712893384


def test_pio2_points_reduce_with_the_intended_n():
    x, n = fp.pio2_points()
    assert n[0] == 1 and n[-1] == 63661 and x[-1] < 1.0e5 < (n[-1] + 1) * np.pi / 2
    np.testing.assert_array_equal(fp.pio2_reduction_n(x), n)
    np.testing.assert_array_equal(fp.pio2_reduction_n(-x), -n)
    # ... and are the nearest doubles: the exact remainder is below half an ulp; it gets as small as 6e-19 (n = 29 2^j)
    with mp.workprec(300):
        rem = [abs(mp.mpf(float(xi)) - int(ni) * mp.pi / 2) for xi, ni in zip(x[::37], n[::37])]
        assert all(r <= mp.mpf(float(np.spacing(xi))) / 2 for r, xi in zip(rem, x[::37]))
        smallest = min(abs(mp.mpf(float(xi)) - int(ni) * mp.pi / 2) for xi, ni in zip(x, n) if ni % 29 == 0 and (ni // 29) & (ni // 29 - 1) == 0)
        assert smallest < 1e-18


def test_threshold_points_have_the_stated_high_words():
    thr = fp.thresholds()
    for word, value in thr.items():
        at, below, same = fp.threshold_points([value])
        assert fp.high_word(at) == word and fp.low_word(at) == 0
        assert below < value and fp.high_word(below) < word and np.nextafter(below, np.inf) == value
        assert fp.high_word(same) == word and fp.low_word(same) != 0 and same > value
    pts = fp.threshold_points([1.5, 6.0], negatives=True)
    np.testing.assert_array_equal(pts[6:], -pts[:6])
    e = fp.sincos_edge_points()
    assert e[0] < 1.0e5 == e[1] < e[2] and fp.high_word(e[0]) < 0x40F86A00
    assert fp.high_word(e[3]) == 0x40F86A00 and fp.low_word(e[3]) != 0


def test_log_points_cover_the_mantissa_interval_ends():
    S = fp.scalars()
    for below_one in (False, True):
        z = fp.log_points(below_one)
        assert z.min() == (np.finfo(np.float64).tiny if below_one else 1.0) and z.max() == np.finfo(np.float64).max
        m, _ = np.frexp(z)
        for n in range(-3, 4):                                        # mantissas within 3 ulp either side of sqrt(1/2)
            assert np.any(m == fp.nudge(S['kSqrtHalf'], n))
        assert np.isin(fp.nudge(1.0, 1), z) and np.isin(fp.nudge(1.0, 4), z) and np.isin(np.ldexp(1.0, 1023), z)
    z = fp.log_points(True)
    assert np.isin(1.0 - 2.0 ** -53, z) and np.isin(2.0 ** -53, z) and np.sum(z < 1.0) > 10000
