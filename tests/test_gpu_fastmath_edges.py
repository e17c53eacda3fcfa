"""The in-kernel elementary functions (csrc/cgp_fastmath.hpp) at the points where they can break -- the ends of the range reductions, the
high-word thresholds that switch regime, the ends of the mantissa interval, subnormal results, wavefronts whose lanes disagree about a
ballot -- in every form a kernel runs, through cgp_debug_math, against mpmath at 200 bits (300 for sin / cos).  The points come from
tests/fastmath_points.py (whose claims test_fastmath_tables.py checks on the CPU); the gates of the lean forms are built per point from
the polynomial errors that module measures.  Each test prints its worst error and where (docs/KERNELS.md holds the table)."""
import functools

import mpmath as mp
import numpy as np
import pytest

from tests import fastmath_points as fp

pytestmark = pytest.mark.gpu

TINY, HUGE = np.finfo(np.float64).tiny, np.finfo(np.float64).max
EPS_SIG_RCP1 = 2.2e-15                          # rcp_nr1, as the header states it


def _dm(op, x):
    from chirpgp_amd import _engine as E
    return E.debug_math(op, np.ascontiguousarray(x, dtype=np.float64))


def _split(want):
    """a list of mpf as two float64 arrays (value = hi + lo to ~ 106 bits): errors against it are then NumPy arithmetic"""
    hi = np.array([float(w) for w in want])
    lo = np.array([float(w - mp.mpf(float(h))) if np.isfinite(h) else 0.0 for w, h in zip(want, hi)])
    return hi, lo


def _err(got, ref):
    """|got - (hi + lo)|: got - hi is exact where the two are within a factor of two, and rounds far below the gates elsewhere"""
    hi, lo = ref
    with np.errstate(invalid='ignore', over='ignore'):
        return np.abs((np.asarray(got) - hi) - lo)


def _ref(f, x, prec=fp.PREC):
    with mp.workprec(prec):
        return _split([f(mp.mpf(float(v))) for v in x])


def _report(what, err, x, scale=None):
    """prints the worst error (relative to `scale` where given) and the point it occurs at"""
    e = np.asarray(err) / (np.abs(scale) if scale is not None else 1.0)
    i = int(np.nanargmax(e))
    print(f'WORST | {what} | {e[i]:.2e} | {float(np.asarray(x).reshape(len(e), -1)[i][0])!r}')


def _softplus(v):
    return mp.log1p(mp.exp(v))


def _sigmoid(v):
    return 1 / (1 + mp.exp(-v))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- exp -----------------------------------------------------------------------------------------------------------------------------
def test_exp_at_the_ends_of_its_reduction_and_into_the_subnormals():
    """fast_exp at the doubles around (k + 1/2) ln 2 for every k a finite result can have, around its two selects, and over (-745.2, -708.4),
    where the result is subnormal: there one unit of 2^-1074 (the single rounding of v_ldexp_f64) on top of the polynomial's 1e-14."""
    x = fp.exp_edge_points()
    got, _ = _dm(0, x)
    with mp.workprec(fp.PREC):
        want = [mp.exp(mp.mpf(float(v))) for v in x]
        top = mp.ldexp(1, 1024) * (1 - mp.ldexp(1, -54))                  # what rounds to +inf
        unit = mp.ldexp(1, -1074)
        over = float(np.float64('709.782712893384'))
        worst_n, worst_s, at_n, at_s = 0.0, 0.0, None, None
        for v, g, w in zip(x, got, want):
            if v > over:
                assert g == np.inf, v
            elif v < -745.2:
                assert g == 0.0, v
            elif np.isinf(g):
                assert w * (1 + mp.mpf('1e-14')) >= top, (v, 'inf where the value is finite')
            else:
                e = abs(mp.mpf(float(g)) - w)
                if w < mp.ldexp(1, -1022):
                    assert e <= unit + mp.mpf('1e-14') * w, (v, g, float(e / unit), 'units of 2^-1074')
                    if float(e / unit) > worst_s:
                        worst_s, at_s = float(e / unit), v
                else:
                    assert e <= mp.mpf('1e-14') * w, (v, g, float(e / w))
                    if float(e / w) > worst_n:
                        worst_n, at_n = float(e / w), v
    print(f'WORST | fast_exp, normal results (relative) | {worst_n:.2e} | {at_n!r}')
    print(f'WORST | fast_exp, subnormal results (units of 2^-1074) | {worst_s:.2e} | {at_s!r}')
    assert np.count_nonzero((got > 0) & (got < TINY)) > 250                 # the subnormal results are there, not flushed


# ---- log, reciprocal, divide ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _log_ref():
    z = fp.log_points(True)
    return z, _ref(mp.log, z)


def _log_gate(z, logz):
    """1e-14 relative; near 1, where log z vanishes, absolute: 1e-14 max(|log z|, |z - 1|)"""
    near = np.abs(z - 1.0) <= 1e-3
    return 1e-14 * np.where(near, np.maximum(np.abs(logz), np.abs(z - 1.0)), np.abs(logz))


def test_log_at_the_ends_of_the_mantissa_interval_and_below_one():
    """fast_log_ge1 on every positive normal argument its callers give it: [1, inf) from the softplus, (0, 1) from the normal generator
    (cgp_rng.hpp: u = 2^-53 (odd)), 2 pi S of either size from nll_increment."""
    z, ref = _log_ref()
    got, _ = _dm(1, z)
    err = _err(got, ref)
    _report('fast_log_ge1, all positive normals (relative; near 1 of max(|log z|, |z - 1|))', err, z, _log_gate(z, ref[0]) / 1e-14 + (z == 1.0))
    assert np.all(err <= _log_gate(z, ref[0])), z[err > _log_gate(z, ref[0])][:5]
    assert got[z == 1.0][0] == 0.0


def test_log_by_direct_exponent_extraction():
    """fast_log_ge1_finite, the lane kernels' form, on [1, 2^1023 sqrt(2)): the same gate.  (Beyond, z sqrt(2) overflows.)"""
    z, ref = _log_ref()
    with np.errstate(over='ignore'):
        keep = (z >= 1.0) & np.isfinite(z * fp.scalars()['kSqrt2'])
    assert keep.sum() > 8000 and z[keep].max() > 1.2e308
    z, ref = z[keep], (ref[0][keep], ref[1][keep])
    got, _ = _dm(18, z)
    err = _err(got, ref)
    _report('fast_log_ge1_finite, [1, 2^1023 sqrt 2) (relative; near 1 of max(|log z|, |z - 1|))', err, z, _log_gate(z, ref[0]) / 1e-14 + (z == 1.0))
    assert np.all(err <= _log_gate(z, ref[0])), z[err > _log_gate(z, ref[0])][:5]
    assert got[z == 1.0][0] == 0.0


def test_reciprocals_at_the_ends_of_the_normal_range_and_their_special_values():
    """rcp_nr, rcp_nr1: 0, +-inf and NaN all give NaN, as the header states; the smallest and the largest normal hold the forms' gates."""
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
    ends = np.array([TINY, -TINY, HUGE, -HUGE, fp.nudge(TINY, 1), fp.nudge(HUGE, -1)])
    for op, gate, name in ((3, 4e-16, 'rcp_nr'), (9, 5e-15, 'rcp_nr1')):
        got, _ = _dm(op, special)
        assert np.isnan(got).all(), (name, got)
        got, _ = _dm(op, ends)
        with mp.workprec(fp.PREC):
            err = np.array([float(abs(mp.mpf(float(g)) * mp.mpf(float(v)) - 1)) for g, v in zip(got, ends)])
        _report(f'{name}, smallest / largest normals (|x r - 1|)', err, ends)
        assert np.all(err < gate), (name, got, err)


def test_divides_to_one_ulp():
    """div_nr, div_nr1: within one ulp of the quotient on random pairs and on pairs whose exact quotient is a double."""
    rng = np.random.default_rng(23)
    n = 10 ** rng.uniform(-100, 100, 5000) * rng.choice([-1, 1], 5000)
    d = 10 ** rng.uniform(-100, 100, 5000) * rng.choice([-1, 1], 5000)
    # exact quotients: q and d of 26 significant bits each, n = q d (exact in float64)
    q = np.ldexp(rng.integers(2 ** 25, 2 ** 26, 2000).astype(np.float64), rng.integers(-60, 60, 2000)) * rng.choice([-1, 1], 2000)
    de = np.ldexp(rng.integers(2 ** 25, 2 ** 26, 2000).astype(np.float64), rng.integers(-60, 60, 2000))
    ne = q * de
    with mp.workprec(fp.PREC):
        assert all(mp.mpf(float(a)) == mp.mpf(float(b)) * mp.mpf(float(c)) for a, b, c in zip(ne[:50], q[:50], de[:50]))
    n, d = np.concatenate([n, ne, [1.0, 3.0, 1.0]]), np.concatenate([d, de, [3.0, 1.0, 10.0]])
    with mp.workprec(fp.PREC):
        ref = _split([mp.mpf(float(a)) / mp.mpf(float(b)) for a, b in zip(n, d)])
    for op, name in ((22, 'div_nr'), (23, 'div_nr1')):
        got, _ = _dm(op, np.stack([n, d], axis=1))
        assert got.shape == n.shape
        err = _err(got, ref) / np.spacing(np.abs(ref[0]))
        _report(f'{name} (ulp of the quotient)', err, n)
        assert np.all(err <= 1.0), (name, n[err > 1.0][:3], d[err > 1.0][:3])
        exact = slice(5000, 7000)
        print(f'{name}: {np.count_nonzero(got[exact] == q)} of 2000 exact quotients returned exactly')


# ---- sin / cos -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pio2_ref():
    x, _ = fp.pio2_points()
    x = np.concatenate([x, fp.sincos_edge_points()])
    with mp.workprec(300):
        cs = [mp.cos_sin(mp.mpf(float(v))) for v in x]
        return x, _split([c[1] for c in cs]), _split([c[0] for c in cs])


@pytest.mark.parametrize('op,name', [(2, 'fast_sincos (fast_sincos_spec)'), (6, 'fast_sincos_uniform, literals'), (17, 'fast_sincos_uniform, FastMathRegs'),
                                     (21, 'fast_sincos_small')])
def test_sincos_at_every_multiple_of_half_pi_below_1e5(op, name):
    """The double nearest n pi/2, n = 1 .. 63 661 (the reduced argument goes down to 6e-19: everything the three-term reduction has to cancel),
    the doubles either side of 1e5 and one with its high word: 3e-16 absolute, and odd / even symmetry bit for bit."""
    x, ref_s, ref_c = _pio2_ref()
    sn, cs = _dm(op, x)
    es, ec = _err(sn, ref_s), _err(cs, ref_c)
    _report(f'{name}: sin at n pi/2 (absolute)', es, x)
    _report(f'{name}: cos at n pi/2 (absolute)', ec, x)
    assert es.max() < 3e-16 and ec.max() < 3e-16, (x[np.argmax(es)], es.max(), x[np.argmax(ec)], ec.max())
    sm, cm = _dm(op, -x)
    np.testing.assert_array_equal(_bits(sm), _bits(-sn))
    np.testing.assert_array_equal(_bits(cm), _bits(cs))


def test_small_angle_sincos_in_wavefronts_that_disagree():
    """fast_sincos_small skips the reduction while a wave-uniform ballot finds every lane within pi/4: wavefronts wholly within 1/4 and
    within pi/4, and ones that one lane -- larger, beyond 1e5, inf, NaN -- sends the long way.  Every lane with |x| <= pi/4 must come out
    with fast_sincos's bits whatever its neighbours do.  (This test found the short series the function once took while every lane was
    within 1/4: one lane in 64 an ulp off.)"""
    rng = np.random.default_rng(29)
    pio4 = fp.scalars()['kPiOver4']
    quarter = np.concatenate([rng.uniform(-0.25, 0.25, 58), [0.25, -0.25, 0.0, -0.0, 1e-300, fp.nudge(0.25, -1)]])
    eighth = np.concatenate([rng.uniform(-pio4, pio4, 58), [pio4, -pio4, fp.nudge(0.25, 1), 0.25, 0.0, fp.nudge(pio4, -1)]])
    waves = [quarter, eighth]
    for base in (quarter, eighth):
        for odd in (fp.nudge(pio4, 1), 3.0, 2.0e5, np.inf, np.nan):
            w = base.copy()
            w[int(rng.integers(0, 64))] = odd
            waves.append(w)
    x = np.concatenate(waves)
    assert x.size % 64 == 0
    sn, cs = _dm(21, x)
    s2, c2 = _dm(2, x)
    fin = np.isfinite(x)
    ref_s, ref_c = _ref(mp.sin, x[fin], 300), _ref(mp.cos, x[fin], 300)
    es, ec = _err(sn[fin], ref_s), _err(cs[fin], ref_c)
    _report('fast_sincos_small in mixed wavefronts: sin (absolute)', es, x[fin])
    _report('fast_sincos_small in mixed wavefronts: cos (absolute)', ec, x[fin])
    assert es.max() < 3e-16 and ec.max() < 3e-16
    assert np.isnan(sn[~fin]).all() and np.isnan(cs[~fin]).all()
    inside = fin & (np.abs(x) <= pio4)
    differ = inside & ((_bits(sn) != _bits(s2)) | (_bits(cs) != _bits(c2)))
    print(f'fast_sincos_small: {np.count_nonzero(differ)} of {np.count_nonzero(inside)} lanes with |x| <= pi/4 differ from fast_sincos; in the all-quarter '
          f'wavefront {np.count_nonzero(differ[:64])}')
    assert not differ.any(), x[differ][:5]


# ---- the softplus forms --------------------------------------------------------------------------------------------------------------
def _grid(lo, hi, n):
    return np.linspace(lo, hi, n)


@functools.lru_cache(maxsize=None)
def _full_points():
    x = np.concatenate([fp.threshold_points([1.5, 6.0, 40.0, 700.0], negatives=True), _grid(-50.0, 60.0, 2200), _grid(60.0, 699.5, 300),
                        [0.0, -0.0, 5.0, 36.7, -36.7, 1e-300]])
    return x, _ref(_softplus, x), _ref(_sigmoid, x)


@pytest.mark.parametrize('op,name', [(20, 'softplus_pair_batch'), (19, 'softplus_batch'), (16, 'softplus_pair_uniform, FastMathRegs'),
                                     (5, 'softplus_pair_uniform, literals'), (4, 'softplus_pair')])
def test_full_accuracy_softplus_forms_at_the_thresholds(op, name):
    """The naive form and the forms that must agree with it: 1e-15 of log1p(exp(x)) and 1e-14 of 1 / (1 + exp(-x)) for x >= 0 (below 0 the
    naive form 1 + exp(x) is itself inaccurate: there, against that form in NumPy, as test_gpu_fastmath.py does), at 1.5, 6, 40, 700 and
    their neighbours."""
    x, ref_sp, ref_d = _full_points()
    sp, dsp = _dm(op, x)
    pos = x >= 0
    e_sp = _err(sp, ref_sp)[pos] / ref_sp[0][pos]
    _report(f'{name}: softplus, x >= 0 (relative)', e_sp, x[pos])
    assert e_sp.max() < 1e-15, x[pos][np.argmax(e_sp)]
    if op != 19:
        e_d = _err(dsp, ref_d)[pos] / ref_d[0][pos]
        _report(f'{name}: derivative, x >= 0 (relative)', e_d, x[pos])
        assert e_d.max() < 1e-14, x[pos][np.argmax(e_d)]
    with np.errstate(over='ignore'):
        e = np.exp(x)
        naive_sp, naive_d = np.log(e + 1.0), e / (e + 1.0)
    neg = (x < 0) & (x >= -30.0)
    assert np.max(np.abs(sp[neg] - naive_sp[neg]) / naive_sp[neg]) < 1e-13
    if op != 19:
        assert np.max(np.abs(dsp[neg] - naive_d[neg]) / naive_d[neg]) < 1e-14
    if op in (5, 16):
        flat = (x >= 40.0) & (x < 700.0)
        assert flat.sum() > 100
        np.testing.assert_array_equal(_bits(sp[flat]), _bits(x[flat]))                      # exactly (x, 1.0) on [40, 700)
        np.testing.assert_array_equal(dsp[flat], np.ones(flat.sum()))


@pytest.mark.parametrize('op', [5, 16])
def test_uniform_pairs_change_form_exactly_at_six(op):
    """Both sides of 6.0 are accurate, so a threshold that moved would pass every gate above; what tells the forms apart is their bits.
    Below 6.0 the wave-uniform pairs ARE softplus_pair (bit for bit, down to the double below 6.0); from 6.0 on they are x + log1p(t) and
    1 / (1 + t), whose roundings differ from the naive form's at a good part of any 200 points -- all of them equal would be the naive form."""
    below = np.concatenate([_grid(5.5, 6.0, 201)[:-1], [float(fp.nudge(6.0, -1)), 1.5, -3.0, 0.0]])
    above = np.concatenate([[6.0, fp.from_words(fp.high_word(6.0), 0x9ABCDEF1)], _grid(6.0, 6.5, 201)[1:-1]])
    (sp, dsp), (sp_n, dsp_n) = _dm(op, below), _dm(4, below)
    np.testing.assert_array_equal(_bits(sp), _bits(sp_n))
    np.testing.assert_array_equal(_bits(dsp), _bits(dsp_n))
    (sp, dsp), (sp_n, dsp_n) = _dm(op, above), _dm(4, above)
    same = (_bits(sp) == _bits(sp_n)) & (_bits(dsp) == _bits(dsp_n))
    print(f'op {op}: {np.count_nonzero(same)} of {same.size} points in [6, 6.5) carry the naive form\'s bits; at 6.0 itself: {bool(same[0])}')
    assert np.count_nonzero(same) < 0.9 * same.size


def test_branch_free_softplus_pair_at_the_thresholds():
    """softplus_pair_any on both sides of 0: 2e-15, and "not valid" from 700 on."""
    x, ref_sp, ref_d = _full_points()
    sp, dsp = _dm(10, x)
    ok = np.abs(x) < 700.0
    assert np.isnan(sp[~ok]).all() and np.isnan(dsp[~ok]).all() and (~ok).sum() == 4
    e_sp, e_d = _err(sp, ref_sp)[ok] / ref_sp[0][ok], _err(dsp, ref_d)[ok] / ref_d[0][ok]
    _report('softplus_pair_any: softplus (relative)', e_sp, x[ok])
    _report('softplus_pair_any: derivative (relative)', e_d, x[ok])
    assert e_sp.max() < 2e-15 and e_d.max() < 2e-15


def test_lane_kernels_softplus_takes_the_naive_form_where_it_must():
    """softplus_pair_batch / softplus_batch: lanes at x >= 700, inf and NaN take softplus_pair's value bit for bit -- in wavefronts that mix
    them with regular lanes, which keep theirs (equal to the all-regular launch)."""
    rng = np.random.default_rng(31)
    regular = rng.uniform(-30.0, 60.0, 256)
    x = regular.copy()
    odd = np.array([700.0, fp.from_words(fp.high_word(700.0), 0x9ABCDEF1), 705.0, 709.7, 709.9, 800.0, 1e4, np.inf, np.nan, fp.nudge(700.0, -1)])
    where = np.array([3, 17, 64, 70, 100, 127, 128, 190, 200, 255])           # all four wavefronts; lane 255 is regular (the double below 700)
    x[where] = odd
    sp_n, d_n = _dm(4, x)
    sp_b, d_b = _dm(20, x)
    sp_1, _ = _dm(19, x)
    beyond = ~(x < 700.0)
    assert beyond.sum() == 9
    for got, want in ((sp_b, sp_n), (d_b, d_n), (sp_1, sp_n)):
        np.testing.assert_array_equal(_bits(got[beyond]), _bits(want[beyond]))
    keep = ~beyond
    keep[where] = False
    sp_r, d_r = _dm(20, regular)
    sp_r1, _ = _dm(19, regular)
    np.testing.assert_array_equal(_bits(sp_b[keep]), _bits(sp_r[keep]))
    np.testing.assert_array_equal(_bits(d_b[keep]), _bits(d_r[keep]))
    np.testing.assert_array_equal(_bits(sp_1[keep]), _bits(sp_r1[keep]))


def _lean_points(lo):
    thr = [v for v in (1.5, 5.0, 6.0, 40.0) if v >= lo]
    pts = fp.threshold_points(thr)
    pts = pts[pts >= lo]
    return np.concatenate([pts, [float(fp.nudge(700.0, -1)), 699.0, 36.7, 37.5], _grid(lo, lo + 3.0, 800), _grid(lo, 60.0, 1500), _grid(60.0, 699.9, 500)])


LEAN_FORMS = [
    # op, name, lower end, negative arguments, (exp, q, sigmoid) errors, one-constant reduction, scales, flat gates of test_gpu_fastmath.py
    (12, 'COMMON step (exp_neg_lean1 + softplus_tail_lean)', 1.5, False, ('exp_lean', 'q_lean', None), True, (1.0, 1.0), True),
    (13, 'LOW step (t = exp(u): t q(t), t / (1 + t))', 1.5, True, ('exp_lean', 'q_lean', None), True, (1.0, 1.0), False),
    (14, 'HIGH step (exp_neg_high + softplus_tail_high, scaled)', 5.0, False, ('exp_high', 'q_high', 'sig_high'), True, (fp.DEBUG_SCALE, fp.DEBUG_DSCALE), False),
    (8, 'lean pair, two-constant reduction', 1.5, False, ('exp_lean', 'q_lean', None), False, (1.0, 1.0), True),
    (7, 'softplus_pair_wide in its regime', 1.5, False, ('exp_lean', 'q_lean', None), False, (1.0, 1.0), True),
]


@pytest.mark.parametrize('op,name,lo,negative,eps,one_constant,scales,flat', LEAN_FORMS, ids=[str(f[0]) for f in LEAN_FORMS])
def test_lean_softplus_forms_point_by_point(op, name, lo, negative, eps, one_constant, scales, flat):
    """The forms the fast kernels run, each held at every point to what its parts allow, with t = exp(-|x|):
        |d sp|  <= 1.25 t (eps_exp + eps_q + eps_red) + 1e-15 |sp|,        |d dsp| <= 1.25 (t eps_exp + eps_sig) + 5e-15 |dsp|
    eps_exp, eps_q (and the HIGH regime's eps_sig) as measured from the tables (fastmath_points.measure), eps_red = |k| 2^-53 ln 2 for the
    one-constant reduction, eps_sig = 2.2e-15 where rcp_nr1 is used; the floors are the uniform form's and rcp_nr1's gates, the 25 % covers
    second-order terms."""
    x = _lean_points(lo)
    x = -x if negative else x
    sp, dsp = _dm(op, x)
    e_exp, e_q = fp.measure(eps[0]), fp.measure(eps[1])
    e_sig = fp.measure(eps[2]) if eps[2] else EPS_SIG_RCP1
    e_red = np.abs(fp.exp_reduction_k(-np.abs(x))) * 2.0 ** -53 * np.log(2.0) if one_constant else 0.0
    with mp.workprec(fp.PREC):
        xs = [mp.mpf(float(v)) for v in x]
        w_sp, w_d = [_softplus(v) for v in xs], [_sigmoid(v) for v in xs]
        d_sp = np.array([float(abs(mp.mpf(float(g)) / mp.mpf(scales[0]) - w)) for g, w in zip(sp, w_sp)])
        d_d = np.array([float(abs(mp.mpf(float(g)) / mp.mpf(scales[1]) - w)) for g, w in zip(dsp, w_d)])
        w_sp, w_d = np.array([float(w) for w in w_sp]), np.array([float(w) for w in w_d])
        t = np.array([float(mp.exp(-abs(v))) for v in xs])
    gate_sp = 1.25 * t * (e_exp + e_q + e_red) + 1e-15 * w_sp
    gate_d = 1.25 * (t * e_exp + e_sig) + 5e-15 * w_d
    _report(f'{name}: softplus (of its gate)', d_sp, x, gate_sp)
    _report(f'{name}: derivative (of its gate)', d_d, x, gate_d)
    _report(f'{name}: softplus (relative)', d_sp, x, w_sp)
    _report(f'{name}: derivative (relative)', d_d, x, w_d)
    assert np.all(d_sp <= gate_sp), (x[d_sp > gate_sp][:5], (d_sp / gate_sp).max())
    assert np.all(d_d <= gate_d), (x[d_d > gate_d][:5], (d_d / gate_d).max())
    if flat:
        assert (d_sp / w_sp).max() < 1e-11 and (d_d / w_d).max() < 2e-11


def test_mid_band_polynomials_with_scales_folded_in():
    """softplus_mid_polys as the MID step runs it, scale and dscale (neither a power of two) in the coefficients and the linear terms: the
    absolute gates of test_gpu_fastmath.py's unscaled pair, times the scale."""
    x = np.concatenate([fp.threshold_points([1.5], negatives=True), [0.0, -0.0, 2.0, -2.0, float(fp.nudge(2.0, -1)), -float(fp.nudge(2.0, -1)), 1e-300, -1e-300,
                                                                      1e-8, -1e-8, 1.75, -1.75], _grid(-2.0, 2.0, 2001)])
    assert np.abs(x).max() <= 2.0
    sp, dsp = _dm(15, x)
    e_sp, e_d = _err(sp, _ref(lambda v: fp.DEBUG_SCALE * _softplus(v), x)), _err(dsp, _ref(lambda v: fp.DEBUG_DSCALE * _sigmoid(v), x))
    _report('MID step, scaled: softplus (absolute / scale)', e_sp / fp.DEBUG_SCALE, x)
    _report('MID step, scaled: derivative (absolute / dscale)', e_d / fp.DEBUG_DSCALE, x)
    assert e_sp.max() < 1e-15 * fp.DEBUG_SCALE and e_d.max() < 5e-16 * fp.DEBUG_DSCALE


# ---- square root, reciprocal root, the likelihood increment -------------------------------------------------------------------------
def test_sqrt_and_reciprocal_root_over_the_whole_range():
    """sqrt_rsqrt: the header's 5e-15 relative on both outputs over 1e-300 .. 1e300; S <= 0 and NaN give NaN."""
    rng = np.random.default_rng(37)
    s = np.concatenate([10 ** rng.uniform(-300, 300, 5000), [1e-300, 1e300, 1.0, 2.0, 4.0, 0.25, 3.0]])
    root, inv = _dm(24, s)
    with mp.workprec(fp.PREC):
        ref = [mp.sqrt(mp.mpf(float(v))) for v in s]
        ref_r, ref_i = _split(ref), _split([1 / r for r in ref])
    e_r, e_i = _err(root, ref_r) / ref_r[0], _err(inv, ref_i) / ref_i[0]
    _report('sqrt_rsqrt: root (relative)', e_r, s)
    _report('sqrt_rsqrt: reciprocal root (relative)', e_i, s)
    assert e_r.max() < 5e-15 and e_i.max() < 5e-15
    root, inv = _dm(24, np.array([0.0, -0.0, -1.0, -1e-300, -np.inf, np.nan]))
    assert np.isnan(root).all() and np.isnan(inv).all()


def test_likelihood_increment_on_both_sides_of_one():
    """nll_increment(S, innov) = (log(2 pi S) + innov^2 / S) / 2 with the engine's own root, reciprocal root and logarithm -- whose argument
    2 pi S is below 1 for S < 0.159.  Gate 1e-14 (1 + |log 2 pi S| + innov^2 / S): the 5e-15 of each root, twice, and the logarithm's 1e-14."""
    rng = np.random.default_rng(41)
    S = np.concatenate([10 ** rng.uniform(-12, 12, 3000), rng.uniform(0.5, 2.0, 2000) / (2 * np.pi), [1 / (2 * np.pi), 0.159, 0.16, 1.0, 1e-12, 1e12]])
    innov = np.sqrt(S) * rng.standard_normal(S.size) * rng.choice([0.0, 1.0, 3.0, 30.0], S.size)
    got, _ = _dm(25, np.stack([S, innov], axis=1))
    with mp.workprec(fp.PREC):
        two_pi = 2 * mp.pi
        lg = [mp.log(two_pi * mp.mpf(float(s))) for s in S]
        qd = [mp.mpf(float(v)) ** 2 / mp.mpf(float(s)) for v, s in zip(innov, S)]
        ref = _split([(a + b) / 2 for a, b in zip(lg, qd)])
        gate = 1e-14 * (1 + np.array([float(abs(a)) for a in lg]) + np.array([float(b) for b in qd]))
    err = _err(got, ref)
    _report('nll_increment (of 1 + |log 2 pi S| + innov^2 / S)', err, S, gate / 1e-14)
    assert np.all(err <= gate), (S[err > gate][:5], innov[err > gate][:5])
    near = np.abs(np.log(2 * np.pi * S)) < 0.7
    assert near.sum() >= 2000
