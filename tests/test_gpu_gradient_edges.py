"""The exact-gradient kernels -- cgp_ekf_nll_grad (csrc/cgp_tangent4.hpp) and cgp_sgp_nll_grad (csrc/cgp_tangent4_sigma.hpp) -- at their
edges, against values and gradients computed in 100-digit arithmetic (tests/golden/exact_grad_cases.npz, written by
tests/golden/make_exact_grad_cases.py): launch shapes beyond one wavefront, record lengths around the measurement chunks, any number of
directions, sigma-point sets of every size class, per-trial operands, shared records, non-finite records, and the parameter region where
the model constants' formulas cancel.

Gates, unless a test says otherwise: value rtol 1e-11, gradient 1e-8 of its largest component (those of test_gpu_gradient.py and
test_gpu_sgp_gradient.py), bit-identity, and 2e-8 where two results are each within 1e-8 of the same exact number.  Every comparison also
prints the error of each gradient component relative to THAT component (floor: 1e-6 of the largest), which the scale metric hides.

RESULTS on an MI355X (every figure below is printed by the tests; none of them set a gate).  Wall time of this file: 3.2 s for its 88
tests (13 s with test_gpu_gradient.py and test_gpu_sgp_gradient.py in the same run).
  * fixture cases, the three cancelling ones aside: cgp_ekf_nll_grad value <= 3.3e-13, gradient <= 7.9e-13 of its scale (random_ekf_21),
    <= 1.3e-12 by component (random_ekf_14); cgp_sgp_nll_grad value <= 4.2e-12 (random_cubature_01), gradient <= 1.6e-9 of its scale and
    <= 1.8e-9 by component (random_gh3_08).
  * lam = 1e-6 / lam = 1e-9 / ell = 30 (value gated against the C port): kernel against port 0 .. 9.4e-15; distance of the value to the exact
    one 9.0e-12 / 7.3e-9 / 2.9e-15 (EKF) and 8.9e-12 / 7.3e-9 / 1.2e-14 (GH-3) -- the port's own, the reference formula's cancellation;
    the port's fourth-order quotient against the exact gradient 7.9e-8 / 6.9e-5 / 3.7e-11 (EKF), 8.3e-8 / 7.3e-5 / 4.2e-10 (GH-3), so
    the gradient gates were 7.9e-7 / 6.9e-4 / 1e-8 and 8.3e-7 / 7.3e-4 / 1e-8; the kernels' gradient errors 2.5e-10 / 2.0e-7 / 3.4e-14 (EKF),
    2.1e-10 / 1.7e-7 / 2.4e-13 (GH-3).
  * record lengths 1 .. 130: value <= 5.5e-16 / 3.9e-14 / 3.5e-15, gradient <= 8.8e-15 / 5.7e-13 / 7.9e-14 (EKF / GH-3 / cubature).
  * direction algebra: copies of a direction in slots of different parity differ by 3.5e-15 of the scale in the GH-3 kernel (0 in the
    cubature run and in the EKF kernel); grad(a d1 + b d2) against a grad(d1) + b grad(d2): <= 2.4e-15 of the scale.
  * on the parent commit's library the T = 0 test fails with `cgp_ekf_nll_grad T = 0: rc 0 nll [nan] grad [nan nan nan nan nan nan]`.
"""
import numpy as np
import numpy.testing as npt
import pytest

from tests import mle_oracle as mo
from tests.tangent_cases import ZG as Z, builder as _builder, directions as _directions, grad_case as _case, raw, run_dirs as _run_dirs, sigma as _sigma

pytestmark = pytest.mark.gpu
NAMES = [str(n) for n in Z['names']]
VALUE_RTOL, GRAD_GATE, PORT_RTOL, TWO_SIDED = 1e-11, 1e-8, 1e-9, 2e-8
CANCELLING = ('lam1e-6', 'lam1e-9', 'ell30')           # the value carries the reference formula's own cancellation: gated against the port
E_UNSUPPORTED = -2


# ------------------------------------------------------------------------------------------------ helpers
def _padded(sg, s):
    """`sg` with zero-weight points at the origin up to s points: they add exact zeros to every sum."""
    from chirpgp_amd.quadratures import SigmaPoints
    n = s - sg.n_points
    return SigmaPoints(4, s, np.r_[np.asarray(sg.w), np.zeros(n)], None, np.vstack([np.asarray(sg.xi), np.zeros((n, 4))]))


def _doubled(sg):
    """every point twice at half its weight: the same rule"""
    from chirpgp_amd.quadratures import SigmaPoints
    return SigmaPoints(4, 2 * sg.n_points, np.repeat(0.5 * np.asarray(sg.w), 2), None, np.repeat(np.asarray(sg.xi), 2, axis=0))


def _vg(c, T=None, sg=None, thetas=None, ys=None, **kw):
    """mle.value_and_grad on a case (its first T measurements; another sigma-point set, parameter vectors or records on request)."""
    from chirpgp_amd import mle
    ys = (c['ys'] if T is None else c['ys'][:T]) if ys is None else ys
    thetas = c['theta'][None, :] if thetas is None else thetas
    sg = _sigma(c['sigma']) if sg is None else sg
    return mle.value_and_grad(_builder(c['build']), thetas, ys, c['Xi'], c['dt'], method=c['method'], sgps=sg, **kw)


def _errors(f, grad, want_f, want_g, label):
    """(value relative error, gradient error over its largest component); prints them and the per-component errors."""
    scale = np.abs(want_g).max()
    ev = abs(f - want_f) / abs(want_f)
    eg = float(np.abs(grad - want_g).max() / scale)
    comp = np.abs(grad - want_g) / np.maximum(np.abs(want_g), 1e-6 * scale)
    print(f'{label}: value error {ev:.2e}, gradient error {eg:.2e} of its scale {scale:.3g}; by component: ' + ' '.join(f'{v:.1e}' for v in comp))
    return ev, eg


def _raw(entry, c, T, dirs, fill, sg=None):
    """The C entry point itself with output buffers pre-filled with `fill`: -> (return code, message, nll (1,), grad (n_dir,))."""
    rc, msg, nll, grad, _ = raw(entry, c, T, dirs, fill, sg=sg)
    return rc, msg, nll, grad[0]


# ------------------------------------------------------------------------------------------------ 0. the fixture holds what it must
def test_the_fixture_holds_every_group():
    """The generator may replace a rejected draw but not drop a case: the counts per group, the dt = 1e-2 and the "lost" cases per method,
    every named edge for both kernels, and no group with more than half its draws rejected."""
    assert int(Z['count.random_ekf']) >= 24 and int(Z['count.random_gh3']) >= 10 and int(Z['count.random_cubature']) >= 6
    assert int(Z['count.prefix']) == 3 and int(Z['count.size']) == 2 and int(Z['count.other']) == 2 and int(Z['count.edge']) == 20
    for grp in ('random_ekf', 'random_gh3', 'random_cubature'):
        cases = [_case(n) for n in NAMES if str(Z[f'{n}.group']) == grp]
        assert sum(c['dt'] == 1e-2 for c in cases) >= 4 and sum(int(c['lost']) for c in cases) >= 4, grp
        assert sum(c['build'] == 'lascala' for c in cases) >= 1, grp
        assert 2 * int(Z[f'rejected.{grp}']) <= int(Z[f'drawn.{grp}']), grp
        assert all(c['moved_nll'] < 1e-13 and c['moved_grad'] < 1e-10 for c in cases), grp
        assert all(40 <= c['ys'].size <= 130 for c in cases)
    for tag in ('ekf', 'gh3'):
        for label in ('lam0', 'lam1e-3', 'lam1e-6', 'lam1e-9', 'ell30', 'ell0.02', 'b1e-4', 'sigma10', 'freq_high', 'freq_low'):
            assert f'edge_{tag}_{label}' in NAMES
        assert Z[f'edge_{tag}_lam0.theta'][0] == -800. and Z[f'edge_{tag}_lam0.grad'][0] == 0.
        assert Z[f'other_{tag}_H_dXi.grad'].size == 7 and not np.array_equal(Z[f'other_{tag}_H_dXi.H'], [0., 1., 0., 0.])
    assert Z['size_gh4.ys'].size == 64 and Z['size_gh5.ys'].size == 40
    for n in ('prefix_ekf', 'prefix_gh3', 'prefix_cubature'):
        assert Z[f'{n}.nll_prefix'].shape == (130,) and Z[f'{n}.grad_prefix'].shape == (130, 6)


# ------------------------------------------------------------------------------------------------ 1. every fixture case
@pytest.mark.parametrize('name', NAMES)
def test_fixture_case(name):
    """Covers: `H`, a non-unit one, and the direction's `dXi` entry (dp[9]) != 0 (other_*_H_dXi, through E.run_*_nll_grad with
    mle.tangent_directions plus the direction whose only entry is dXi = 1); sigma sets with s > 128 (size_gh4 = 256, size_gh5 = 625 points:
    points re-evaluated in every pass); the host directions away from the fixtures' point carried through the scan (edge_*); dt = 1e-2, the
    lost filter, the La Scala builder (random_*).

    Gates: value 1e-11, gradient 1e-8 of its scale.  Named parameter edges: for lam = 1e-6, 1e-9 and ell = 30 the VALUE carries the reference
    formula's own cancellation (q, M32_Sigma: in the port as well), so the value is gated against the C port (rtol 1e-9, the project's
    parity gate), its distance to the exact value is printed, and the gradient gate is the larger of 1e-8 and ten times the error of the
    PORT's fourth-order quotient against the exact gradient; for the other named edges the gates are the fixed ones or, where larger, 100
    times the movement of the exact value / gradient under the generator's 1e-15 perturbation."""
    c = _case(name)
    build, sg = _builder(c['build']), _sigma(c['sigma'])
    if int(c['with_dxi']):
        d7 = np.zeros((1, 1, 24))
        d7[0, 0, 9] = 1.0
        f, grad = _run_dirs(c, np.concatenate([_directions(c), d7], axis=1), H=c['H'])
    else:
        f, grad = _vg(c)
    ev, eg = _errors(f[0], grad[0], c['nll'], c['grad'], name)
    value_gate, grad_gate = VALUE_RTOL, GRAD_GATE
    if c['group'] == 'edge':
        if name.split('_', 2)[2] in CANCELLING:
            port_f, port_g = mo.value_and_grad(c['method'], build, c['theta'], c['ys'], c['Xi'], c['dt'], sgps=sg)
            port_err = float(np.abs(port_g - c['grad']).max() / np.abs(c['grad']).max())
            grad_gate = max(GRAD_GATE, 10.0 * port_err)
            print(f'   value against the port {abs(f[0] - port_f) / abs(port_f):.2e}; port against exact {abs(port_f - c["nll"]) / abs(c["nll"]):.2e}; '
                  f"port's quotient against the exact gradient {port_err:.2e} -> gradient gate {grad_gate:.2e}")
            npt.assert_allclose(f[0], port_f, rtol=PORT_RTOL)
            assert eg < grad_gate, (grad, c['grad'])
            return
        value_gate, grad_gate = max(VALUE_RTOL, 100.0 * c['moved_nll']), max(GRAD_GATE, 100.0 * c['moved_grad'])
        print(f'   moved by {c["moved_nll"]:.2e} / {c["moved_grad"]:.2e} under the 1e-15 perturbation -> gates {value_gate:.2e} / {grad_gate:.2e}')
    assert ev < value_gate, (f[0], c['nll'])
    assert eg < grad_gate, (grad, c['grad'])


# ------------------------------------------------------------------------------------------------ 2. record lengths
@pytest.mark.parametrize('name', ['prefix_ekf', 'prefix_gh3', 'prefix_cubature'])
def test_record_lengths(name):
    """Covers: EKF tangent, measurements fetched 8 steps at a time with a zero-filled tail (T = 1, 2, 7, 8, 9); SGP tangent, 64-step
    measurement chunks by readlane (T = 1, 63, 64, 65, 127, 128, 129) -- both kernels at all of them, against the 100-digit value and
    gradient of every prefix of one record."""
    c = _case(name)
    want_f, want_g = Z[f'{name}.nll_prefix'], Z[f'{name}.grad_prefix']
    worst = [0., 0.]
    for T in (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 130):
        f, grad = _vg(c, T=T)
        ev, eg = _errors(f[0], grad[0], want_f[T - 1], want_g[T - 1], f'{name} T = {T}')
        worst = [max(worst[0], ev), max(worst[1], eg)]
        assert ev < VALUE_RTOL and eg < GRAD_GATE, (T, f[0], want_f[T - 1], grad[0], want_g[T - 1])
    print(f'{name}: worst over the record lengths: value {worst[0]:.2e}, gradient {worst[1]:.2e}')


@pytest.mark.parametrize('entry', ['cgp_ekf_nll_grad', 'cgp_sgp_nll_grad'])
def test_an_empty_record_writes_zeros(entry):
    """Covers: `launch_ekf4_tangent` returned without a launch at T = 0 while the entry point returned OK, so `nll` and `grad` stayed the
    caller's unwritten memory.  Both entry points, output buffers pre-filled with NaN: nll == 0 and grad == 0 exactly."""
    c = _case('prefix_ekf' if entry == 'cgp_ekf_nll_grad' else 'prefix_gh3')
    dirs = _directions(c)[0]
    rc, msg, nll, grad = _raw(entry, c, 0, dirs, np.nan, sg=_sigma(c['sigma']))
    print(entry, 'T = 0: rc', rc, 'nll', nll, 'grad', grad)
    assert rc == 0, msg
    assert np.array_equal(nll, [0.0]) and np.array_equal(grad, np.zeros(6))
    f, g_ = _vg(c, ys=np.zeros(0))
    assert np.array_equal(f, [0.0]) and np.array_equal(g_, np.zeros((1, 6)))


# ------------------------------------------------------------------------------------------------ 3. launch shapes
def _chirp_thetas():
    """The parameter vectors of the random chirp cases of the EKF group, and the prefix case's (row 0)."""
    rows = [Z['prefix_ekf.theta']] + [Z[f'{n}.theta'] for n in NAMES if n.startswith('random_ekf') and str(Z[f'{n}.build']) == 'chirp']
    return np.stack(rows)


def _three_records():
    ys = Z['prefix_ekf.ys']
    rng = np.random.default_rng(31)
    return np.stack([ys, ys[::-1].copy(), 0.7 * ys + 0.3 * rng.standard_normal(ys.size)])


@pytest.mark.parametrize('name', ['prefix_ekf', 'prefix_gh3', 'prefix_cubature'])
def test_seven_hundred_trials_in_one_launch(name):
    """Covers: EKF tangent, lane = trial * n_dir + direction, 64 lanes a block -- 4200 lanes in 66 blocks, trials whose directions straddle
    two wavefronts, the partial last block; SGP tangent: 700 blocks; `ys_repeat` (7) with a permuted, repeating `ys_index` (100 entries
    over three records).  Every row bit-identical to the same trial launched alone; the rows that are the prefix case within the gates."""
    c = _case(name)
    thetas, recs = _chirp_thetas(), _three_records()
    rng = np.random.default_rng(700)
    index = rng.permutation(np.arange(100) % 3)
    pick = rng.integers(0, thetas.shape[0], size=700)
    pick[::50] = 0                                                   # the prefix case's parameters on whatever record the row has
    f, grad = _vg(c, thetas=thetas[pick], ys=recs, record_index=index)
    assert f.shape == (700,) and grad.shape == (700, 6)
    alone = {}
    fixture_rows = 0
    for t in range(700):
        key = (int(pick[t]), int(index[t // 7]))
        if key not in alone:
            alone[key] = _vg(c, thetas=thetas[key[0]][None, :], ys=recs[key[1]])
        npt.assert_array_equal(f[t], alone[key][0][0], err_msg=f'trial {t} {key}')
        npt.assert_array_equal(grad[t], alone[key][1][0], err_msg=f'trial {t} {key}')
        if key == (0, 0):
            fixture_rows += 1
            ev = abs(f[t] - c['nll']) / abs(c['nll'])
            eg = np.abs(grad[t] - c['grad']).max() / np.abs(c['grad']).max()
            assert ev < VALUE_RTOL and eg < GRAD_GATE, (t, ev, eg)
    assert fixture_rows >= 1
    print(f'{name}: 700 trials, {len(alone)} distinct (parameters, record) pairs, {fixture_rows} fixture rows: every row bit-identical to its lone launch')
    # ---- the straddling trial (trial 10 at n_dir = 6 owns lanes 60 .. 65) absent, last, inside
    for B in (10, 11, 12):
        fB, gB = _vg(c, thetas=thetas[:B], ys=recs[0])
        for t in range(B):
            key = (t, 0)
            if key not in alone:
                alone[key] = _vg(c, thetas=thetas[t][None, :], ys=recs[0])
            npt.assert_array_equal(fB[t], alone[key][0][0], err_msg=f'B = {B} trial {t}')
            npt.assert_array_equal(gB[t], alone[key][1][0], err_msg=f'B = {B} trial {t}')


@pytest.mark.parametrize('name', ['prefix_ekf', 'prefix_gh3'])
def test_per_trial_operands(name):
    """Covers: `H`, `Xi`, `m0`, `P0` with per-trial strides (B values each, non-unit H): bit-identical to the same trials launched one by
    one with scalars."""
    c = _case(name)
    B, T = 5, 65
    rng = np.random.default_rng(55)
    thetas = _chirp_thetas()[:B]
    dirs = _directions(c, thetas)
    H = rng.uniform(-1.5, 1.5, size=(B, 4))
    Xi = 10 ** rng.uniform(-2, 0, size=B)
    m0 = rng.uniform(-1, 1, size=(B, 4)) + np.array([0., 0., 7., 0.])
    A = rng.uniform(-0.3, 0.3, size=(B, 4, 4))
    P0 = np.eye(4)[None] * rng.uniform(0.1, 1.0, size=(B, 4))[:, None, :] + A @ A.transpose(0, 2, 1)
    f, grad = _run_dirs(c, dirs, T=T, H=H, Xi=Xi, m0=m0, P0=P0, thetas=thetas, trials_per_record=B)
    assert np.isfinite(f).all() and np.isfinite(grad).all()
    assert len({float(v) for v in f}) == B
    for i in range(B):
        fi, gi = _run_dirs(c, dirs[i:i + 1], T=T, H=H[i], Xi=float(Xi[i]), m0=m0[i], P0=P0[i], thetas=thetas[i:i + 1])
        npt.assert_array_equal(fi[0], f[i])
        npt.assert_array_equal(gi[0], grad[i])


# ------------------------------------------------------------------------------------------------ 4. direction algebra
N_DIRS = (1, 2, 3, 5, 6, 7, 15, 16, 17, 33)


def _layout(n_dir):
    """Which of the six parameter directions sits in slot j (-1: an all-zero direction): the six in order, a zero after every sixth."""
    return [-1 if j % 7 == 6 else (j - j // 7) % 6 for j in range(n_dir)]


@pytest.mark.parametrize('name', ['prefix_ekf', 'prefix_gh3', 'prefix_cubature'])
def test_direction_algebra(name):
    """Covers: SGP tangent, passes of two directions, npass = 1 + nd / 2, pass / slot by lane parity -- odd nd (1, 3, 5, 15), nd = 16 (the
    last table row), n_dir > 16 (slices with dir0 > 0); and the EKF kernel's lane = trial * n_dir + direction at every n_dir.
    The ABI takes any directions: a zero direction gives exactly 0.0; copies of a direction give bit-identical results in whatever slot
    and slice they sit; slots 0 .. 5 meet the fixture gate at every n_dir; a direction scaled by 4 and by 0.5 in the same slot of a second
    launch gives the result scaled bit for bit; grad(a d1 + b d2) = a grad(d1) + b grad(d2) within 2e-8 of the scale; nll is bit-identical
    for every n_dir.

    The sigma-point kernel's two inlined copies of FanPoint::add_tangent (slot A / slot B of a pass; odd / even lane) are contracted into
    different fused multiply-adds -- in the gfx950 disassembly of sgp4_tangent_kernel slot A accumulates the mean sums as
    v_fma_f64(w, df, acc) where slot B multiplies (v_mul_f64 w, df) and adds (v_add_f64) -- so a direction's result depends on its slot's
    parity in the last bits (2.6e-18 absolute on direction 0, GH-3).  Copies in slots of different parity are therefore compared within
    2e-8 of the scale (each is within 1e-8 of the same exact number); copies in slots of the same parity, and the same slot across slices
    and launches, stay bit-identical.  The EKF kernel has one copy: bit-identical in every slot."""
    c = _case(name)
    T = 65
    want_f, want_g = Z[f'{name}.nll_prefix'][T - 1], Z[f'{name}.grad_prefix'][T - 1]
    scale = np.abs(want_g).max()
    base = _directions(c)[0]                                          # (6, 24)
    first, same, across = {}, {}, 0.0
    split_parity = c['method'] == 'sgp_filter'
    nll0 = None
    for n_dir in N_DIRS:
        lay = _layout(n_dir)
        dirs = np.stack([np.zeros(24) if k < 0 else base[k] for k in lay])[None]
        f, grad = _run_dirs(c, dirs, T=T)
        nll0 = f[0] if nll0 is None else nll0
        npt.assert_array_equal(f[0], nll0, err_msg=f'nll at n_dir = {n_dir}')
        assert abs(f[0] - want_f) / abs(want_f) < VALUE_RTOL
        for j, k in enumerate(lay):
            if k < 0:
                assert grad[0, j] == 0.0, (n_dir, j, grad[0, j])
                continue
            first.setdefault(k, (grad[0, j], n_dir, j))
            key = (k, j & 1) if split_parity else (k, 0)
            same.setdefault(key, (grad[0, j], n_dir, j))
            npt.assert_array_equal(grad[0, j], same[key][0], err_msg=f'direction {k} in slot {j} of n_dir = {n_dir} against slot {same[key][2]} of n_dir = {same[key][1]}')
            across = max(across, abs(grad[0, j] - first[k][0]) / scale)
            assert abs(grad[0, j] - first[k][0]) <= TWO_SIDED * scale, (n_dir, j, k)
        m = min(n_dir, 6)
        eg = np.abs(grad[0, :m] - want_g[:m]).max() / scale
        assert eg < GRAD_GATE, (n_dir, eg)
        # ---- scaled by a power of two in the same slots of a second launch: scaled bit for bit
        for a in (4.0, 0.5):
            f2, g2 = _run_dirs(c, a * dirs, T=T)
            npt.assert_array_equal(f2[0], nll0)
            npt.assert_array_equal(g2[0], a * grad[0], err_msg=f'directions scaled by {a} at n_dir = {n_dir}')
    _errors(nll0, np.array([first[k][0] for k in range(6)]), want_f, want_g, f'{name} T = {T}, any n_dir')
    print(f'{name}: copies of a direction in slots of different parity differ by at most {across:.2e} of the scale')
    # ---- linearity in the direction: |a| + |b| = 1, so each side is within 1e-8 of the scale of the same exact number
    rng = np.random.default_rng(4)
    g6 = np.array([first[k][0] for k in range(6)])
    combos = np.zeros((6, 6))
    for r in range(6):
        i, j = rng.choice(6, size=2, replace=False)
        a = rng.uniform(0.1, 0.9)
        combos[r, i], combos[r, j] = a, (a - 1.0 if r % 2 else 1.0 - a)
    f, grad = _run_dirs(c, (combos @ base)[None], T=T)
    lin = np.abs(grad[0] - combos @ g6).max() / scale
    print(f'{name}: grad(a d1 + b d2) against a grad(d1) + b grad(d2): {lin:.2e} of the scale (six random pairs)')
    assert lin < TWO_SIDED


# ------------------------------------------------------------------------------------------------ 5. sigma-set sizes
@pytest.mark.parametrize('name,sizes', [('prefix_cubature', (9, 32, 33, 64, 65, 128, 129, 130)), ('prefix_gh3', (128, 129, 130))])
def test_sigma_set_sizes(name, sizes):
    """Covers: SGP tangent, points two per lane, kept when s <= 128, re-evaluated in every pass when s > 128; the `narrow` reduction when
    s <= 32 -- s in 33 .. 64, 64 / 65, 128 / 129 (GH-4 = 256 and GH-5 = 625 points are fixture cases of their own: test_fixture_case).
    The cubature rule (8 points) and GH-3 (81) padded with zero-weight points at the origin, and with every point doubled at half weight
    (s = 16, 162): the same rule, so the unpadded rule's 100-digit values within the gates."""
    c = _case(name)
    T = 64
    want_f, want_g = Z[f'{name}.nll_prefix'][T - 1], Z[f'{name}.grad_prefix'][T - 1]
    sg = _sigma(c['sigma'])
    sets = [(f's = {s} (padded)', _padded(sg, s)) for s in sizes] + [(f's = {2 * sg.n_points} (doubled)', _doubled(sg))]
    for label, sgp in sets:
        f, grad = _vg(c, T=T, sg=sgp)
        ev, eg = _errors(f[0], grad[0], want_f, want_g, f'{name} {label}')
        assert ev < VALUE_RTOL and eg < GRAD_GATE, (label, f[0], want_f, grad[0], want_g)


def test_a_set_beyond_the_lds_stage_is_refused():
    """Covers: the LDS-stage refusal (GH-6 = 1296 points): CGP_E_UNSUPPORTED with the LDS-stage message, the outputs untouched."""
    from chirpgp_amd.quadratures import SigmaPoints
    c = _case('prefix_gh3')
    sg = SigmaPoints.gauss_hermite(4, 6)
    assert sg.n_points == 1296
    rc, msg, nll, grad = _raw('cgp_sgp_nll_grad', c, 40, _directions(c)[0], 123.0, sg=sg)
    assert rc == E_UNSUPPORTED and b'LDS stage' in msg, (rc, msg)
    assert np.array_equal(nll, [123.0]) and np.array_equal(grad, np.full(6, 123.0))


# ------------------------------------------------------------------------------------------------ 6. non-finite records
@pytest.mark.parametrize('name', ['prefix_ekf', 'prefix_gh3'])
@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_non_finite_records(name, bad):
    """Covers: NaN or inf in a record -- at step 0, at step 70 and at the last step of one trial of five.  That trial's nll is NaN exactly
    where the C port's final NLL is NaN, and then every entry of its grad is NaN; the other four trials are bit-identical to the launch
    without the bad value; make_objective(..., exact=True) returns (inf, zeros) on it."""
    from chirpgp_amd import mle
    c = _case(name)
    build, sg = _builder(c['build']), _sigma(c['sigma'])
    rng = np.random.default_rng(6)
    recs = c['ys'][None, :] * rng.uniform(0.8, 1.2, size=(5, 1)) + 0.05 * rng.standard_normal((5, c['ys'].size))
    thetas = np.repeat(c['theta'][None, :], 5, axis=0)
    clean_f, clean_g = _vg(c, thetas=thetas, ys=recs)
    assert np.isfinite(clean_f).all() and np.isfinite(clean_g).all()
    for step in (0, 70, recs.shape[1] - 1):
        trial = 2
        ys = recs.copy()
        ys[trial, step] = bad
        f, grad = _vg(c, thetas=thetas, ys=ys)
        port = mo.nll(c['method'], build, c['theta'][None, :], ys[trial], c['Xi'], c['dt'], sgps=sg)[0]
        print(f'{name}: {bad} at step {step}: nll {f[trial]}, port {port}, grad {grad[trial]}')
        assert np.isnan(f[trial]) == np.isnan(port)
        if np.isnan(f[trial]):
            assert np.isnan(grad[trial]).all()
        keep = np.arange(5) != trial
        npt.assert_array_equal(f[keep], clean_f[keep])
        npt.assert_array_equal(grad[keep], clean_g[keep])
        assert not np.isfinite(f[trial])
        v, g_ = mle.make_objective(c['method'], build, ys[trial], c['Xi'], c['dt'], sgps=sg, exact=True)(c['theta'])
        assert v == np.inf and np.array_equal(g_, np.zeros(6))
