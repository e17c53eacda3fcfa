"""`substeps=n` (CGP_RK4_SUBSTEPS, include/chirpgp_hip.h) without a GPU: the refined-grid oracle that defines it (tests/substeps_oracle.py),
what n buys on a coarsely sampled record, the macro and its Python mirror, and -- through the host probes tests/route_probe.hip and
tests/abi_probe.hip -- that a flagged call only reaches a kernel that honours the flag and that everything else refuses it.

The records: sin(2 pi (f0 t + t^2)) + noise of variance 0.1, t = dt, 2 dt, ..., 150 samples at dt = 1e-2, numpy's default_rng(1);
the chirp model started at f0.  At f0 = 20 Hz (2 pi f dt = 1.26) one RK4 step per sample is inside its stability region and far from the
ODE's answer: the final NLL of cd_ekf is 276.3 with n = 1, 366.7 with n = 4, 371.4 with n = 8.  At f0 = 60 Hz (3.77) it is outside: NaN with
n = 1 and 2, 375.4 with n = 4, 394.6 with n = 8."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import np_filters as onp
from oracle import np_models as om
from oracle.np_quadratures import SigmaPoints as OSigmaPoints
from tests import abi_cases as ac
from tests import route_cases as rc
from tests import substeps_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, XI = 1e-2, 0.1


def SUB(n):
    return (n - 1) << 16                                  # CGP_RK4_SUBSTEPS(n)


def filtered(n, f0, fn=None, *sigma):
    """(cumulative NLL, filtering means) of an oracle filter (cd_ekf) with n substeps on the f0 record."""
    drift, disp, _, m0, P0, H = so.chirp_model(f0)
    (mfs, _, nll), _ = so.run_filter(fn or onp.cd_ekf, n, drift, disp(None) if sigma else disp, *sigma, H, XI, m0, P0, DT, so.chirp_record(f0))
    return nll, mfs


# ---- the definition

def test_one_substep_is_the_plain_oracle_bit_for_bit():
    drift, disp, _, m0, P0, H = so.chirp_model(20.)
    ys = so.chirp_record(20., T=40)
    sg = OSigmaPoints.gauss_hermite(4, 3)
    for fn, sm, head, b in ((onp.cd_ekf, onp.cd_eks, (), disp), (onp.cd_sgp_filter, onp.cd_sgp_smoother, (sg,), disp(None))):
        kept, full = so.run_filter(fn, 1, drift, b, *head, H, XI, m0, P0, DT, ys)
        plain = fn(drift, b, *head, H, XI, m0, P0, DT, ys)
        for got, all_rows, want in zip(kept, full, plain):
            assert np.array_equal(got, want, equal_nan=True) and np.array_equal(all_rows, want, equal_nan=True)
        got_s = so.run_smoother(sm, 1, drift, b, *head, full[0], full[1], DT)
        want_s = sm(drift, b, *head, plain[0], plain[1], DT)
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got_s, want_s))      # (NaN and all: n = 1 is unstable on this record)


def test_refined_record_and_kept_rows():
    ys = np.arange(1., 6.)
    for n in (1, 2, 3, 16):
        ref = so.refine(ys, n)
        assert ref.shape == (5 * n,) and np.array_equal(ref[so.kept(n)], ys) and np.isnan(ref).sum() == 5 * (n - 1)
        assert list(range(5 * n))[so.kept(n)] == [n - 1 + k * n for k in range(5)]


def test_the_issues_figures():
    """The records and the model are the ones the figures in the docstring were taken on."""
    got = [round(float(filtered(n, 20.)[0][-1]), 1) for n in (1, 4, 8)]
    assert got == [276.3, 366.7, 371.4], got


def test_fourth_order_inside_the_stability_region():
    """RK4 is fourth order: the distance of cd_ekf's filtering means to the n = 16 result -- the largest difference of a component over the
    record -- falls by a factor of at least 8 each time n doubles from 2 to 8 (16 in the limit; 12.5 and 33.4 here)."""
    ref = filtered(16, 20.)[1]
    d = {n: float(np.max(np.abs(filtered(n, 20.)[1] - ref))) for n in (1, 2, 4, 8)}
    print('distance to n = 16:', d)
    assert d[2] >= 8 * d[4] and d[4] >= 8 * d[8], d
    assert d[1] > 2.5 and d[4] < 0.2, d                   # 2.9 and 0.18: one step per sample is far from the ODE's answer


def test_instability_rescued():
    """2 pi f dt = 3.77 is outside RK4's stability region: the NLL ends in NaN with one or two steps per sample, finite with four and eight.
    The sigma-point filter breaks down earlier: NaN with one step at 20 Hz already, finite with two."""
    for n, finite in ((1, False), (2, False), (4, True), (8, True)):
        assert math.isfinite(filtered(n, 60.)[0][-1]) == finite, n
    assert [round(float(filtered(n, 60.)[0][-1]), 1) for n in (4, 8)] == [375.4, 394.6]
    sg = OSigmaPoints.gauss_hermite(4, 3)
    assert math.isnan(filtered(1, 20., onp.cd_sgp_filter, sg)[0][-1]) and math.isfinite(filtered(2, 20., onp.cd_sgp_filter, sg)[0][-1])


def test_real_gaps_on_top():
    """A NaN of the caller's record is a gap of the refined one like the inserted ones: n = 1 with gaps is tests/gap_oracle.py's filter."""
    from tests import gap_oracle as go
    drift, disp, _, m0, P0, H = so.chirp_model(20.)
    ys = go.with_gaps(so.chirp_record(20., T=40), ((3, 5), (39, 40)))
    kept, _ = so.run_filter(onp.cd_ekf, 1, drift, disp, H, XI, m0, P0, DT, ys)
    want = go.gapped(onp.cd_ekf, drift, disp, H, XI, m0, P0, DT, ys)
    assert all(np.array_equal(g, w) for g, w in zip(kept, want))
    kept3, _ = so.run_filter(onp.cd_ekf, 3, drift, disp, H, XI, m0, P0, DT, ys)
    assert np.isfinite(kept3[0]).all() and kept3[2][3] == kept3[2][2] == kept3[2][4]      # the NLL holds over the gap


# ---- the macro and its mirror

def test_header_declares_the_macro_and_the_engine_mirrors_it():
    from chirpgp_amd import _engine as E
    with open(os.path.join(ROOT, 'include', 'chirpgp_hip.h')) as fh:
        src = fh.read()
    assert re.search(r'#define\s+CGP_RK4_SUBSTEPS\(n\)\s+\(\(uint32_t\)\(\(n\) - 1\) << 16\)', src)
    mask = re.search(r'#define\s+CGP_RK4_SUBSTEPS_MASK\s+(0x[0-9A-Fa-f]+)u', src)
    assert mask and int(mask.group(1), 16) == 0x000F0000 == E.RK4_SUBSTEPS_MASK
    assert E.rk4_substeps(1) == 0 and E.MAX_SUBSTEPS == 16
    for n in range(1, 17):
        assert E.rk4_substeps(n) == SUB(n) and SUB(n) & ~E.RK4_SUBSTEPS_MASK == 0
    assert SUB(17) & ~E.RK4_SUBSTEPS_MASK                 # n = 17 cannot be encoded ...
    for bad in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError):                   # ... and the Python layer says so
            E.rk4_substeps(bad)
    # no other flag of the header lives in those bits
    others = [int(v, 16) for name, v in re.findall(r'#define\s+(CGP_[A-Z_0-9]+)\s+(0x[0-9A-Fa-f]+)u\b', src)
              if not name.startswith(('CGP_SIGMA_', 'CGP_RK4_'))]
    assert others and not any(v & E.RK4_SUBSTEPS_MASK for v in others)


def test_python_refuses_before_anything_is_launched():
    """A discrete method or model (a run-time compiled one included), a time split or a count outside 1 .. 16: ValueError, before torch is even
    imported."""
    from chirpgp_amd import _engine as E
    z = np.zeros(4)
    with pytest.raises(ValueError, match='continuous-discrete'):
        E.run_filter(E.F_EKF, None, None, None, z, 0.1, z, np.eye(4), 1e-3, z, substeps=2)
    with pytest.raises(ValueError, match='continuous-discrete'):
        E.run_smoother(E.S_SGP, None, None, None, 1e-3, np.zeros((3, 4)), np.zeros((3, 4, 4)), substeps=2)
    with pytest.raises(ValueError, match='time_split'):
        E.run_filter(E.F_CD_SGP, None, None, None, z, 0.1, z, np.eye(4), 1e-3, z, substeps=2, time_split=(2, 64))
    with pytest.raises(ValueError, match='time_split'):
        E.run_smoother(E.S_CD_EKS, None, None, None, 1e-3, np.zeros((3, 4)), np.zeros((3, 4, 4)), substeps=4, time_split=(2, 64))
    with pytest.raises(ValueError, match='1 .. 16'):
        E.run_filter(E.F_CD_EKF, None, None, None, z, 0.1, z, np.eye(4), 1e-3, z, substeps=17)
    with pytest.raises(ValueError, match='1 .. 16'):
        E.run_smoother(E.S_CD_EKS, None, None, None, 1e-3, np.zeros((3, 4)), np.zeros((3, 4, 4)), substeps=0)
    with pytest.raises(ValueError, match='continuous-discrete'):      # (no custom_sde model)
        E.run_filter_custom(None, None, z, 0.1, z, np.eye(4), 1e-3, z, substeps=2)
    with pytest.raises(ValueError, match='continuous-discrete'):      # (no custom_sde model)
        E.run_smoother_custom(None, None, 1e-3, np.zeros((3, 4)), np.zeros((3, 4, 4)), substeps=2)


def test_mle_refuses_before_anything_is_built():
    """mle: substeps > 1 with a discrete method -- whichever form of the gradient -- or a count outside 1 .. 16 is a ValueError before the
    builder is even called; the exact gradient takes them for 'cd_ekf', which has one, and 'cd_sgp_filter' has none with or without."""
    from chirpgp_amd import mle

    def build(*a, **k):
        raise AssertionError('the builder was called')
    th, ys = np.zeros((1, 6)), np.zeros(8)
    for method in ('ekf', 'sgp_filter', 'ekf_for_kpt'):
        with pytest.raises(ValueError, match='substeps'):
            mle.batched_nll(method, build, th, ys, XI, DT, substeps=2)
        with pytest.raises(ValueError, match='substeps'):
            mle.fit(method, build, [1.] * 6, ys, XI, DT, substeps=2)
        with pytest.raises(ValueError, match='substeps'):
            mle.fit_many(method, build, [1.] * 6, ys, XI, DT, substeps=2)
        with pytest.raises(ValueError, match='substeps'):
            mle.grid_search(method, build, np.ones((2, 6)), ys, XI, DT, substeps=2)
    for bad in (0, 17):
        with pytest.raises(ValueError, match='1 .. 16'):
            mle.batched_nll('cd_ekf', build, th, ys, XI, DT, substeps=bad)
    for method in ('ekf', 'sgp_filter'):                  # the exact gradient takes substeps for 'cd_ekf' alone
        with pytest.raises(ValueError, match='substeps'):
            mle.value_and_grad(build, th, ys, XI, DT, method=method, substeps=4)
    with pytest.raises(ValueError, match='1 .. 16'):
        mle.value_and_grad(build, th, ys, XI, DT, method='cd_ekf', substeps=17)
    with pytest.raises(ValueError, match='exact=True'):   # cd_sgp_filter has no tangent kernel, with substeps or without
        mle.make_objective('cd_sgp_filter', pm_build(), ys, XI, DT, exact=True, substeps=4)


def pm_build():
    from chirpgp_amd import models as pm
    return pm.build_chirp_model


def test_float64_tangent_oracle_reaches_the_gates_on_the_fixture():
    """tests/golden/exact_cd_substeps.npz (100 digits; both builders, n = 2, 3, 4, T <= 40, two cases with gaps of their own, admitted under
    make_exact_cd_grad.py's rule) against the float64 restatement on the refined record: value 1e-11 relative, gradient 1e-8 of its scale."""
    from tests import cd_grad_cases as cg
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'exact_cd_substeps.npz'))
    names = [str(n) for n in z['names']]
    assert len(names) >= 5 and {str(z[f'{n}.build']) for n in names} == {'chirp', 'lascala'} and {int(z[f'{n}.n']) for n in names} == {2, 3, 4}
    assert any(int(z[f'{n}.skip']) for n in names)
    for n in names:
        assert float(z[f'{n}.moved_nll']) < cg.VALUE_MOVE_MAX and float(z[f'{n}.moved_grad']) < cg.GRAD_MOVE_MAX and len(z[f'{n}.ys']) <= 40
        assert bool(int(z[f'{n}.skip'])) == bool(np.isnan(z[f'{n}.ys']).any())
        f, grad = so.value_and_grad(str(z[f'{n}.build']), z[f'{n}.theta'], z[f'{n}.ys'], float(z[f'{n}.Xi']), float(z[f'{n}.dt']), int(z[f'{n}.n']), H=z[f'{n}.H'])
        ev, eg = cg.errors(f, grad, float(z[f'{n}.nll']), z[f'{n}.grad'], n)
        assert ev <= cg.VALUE_RTOL and eg <= cg.GRAD_GATE


# ---- routes: a flagged call only reaches a kernel that honours the flag (csrc/cgp_route.hpp: honours_substeps)

def q(method, model, sigma=None, B=4, T=128, flags=0, entry='filter', segments=1, n=4, null_rows=False):
    # (a dict of our own: route_cases.case() would append to the pinned list)
    return dict(entry=entry, method=method, model=model, sigma=sigma, B=B, T=T, flags=flags | SUB(n), segments=segments, align=0, num_cus=256,
                null_rows=null_rows)


SMOOTHER_PLAN = ' wave=1 segs=1 tiles=0 bsegs=1 chunks=0 burn=0 sel='
ROUTES = {
    # filters: the d = 4 matrix-core kernels (their SUB instantiations, with gaps or without), else the generic kernel in the shape the call has
    'cd_ekf-chirp': (q('cd_ekf', 'chirp_sde1'), 'cdekf4_mfma wave=1 segs=1'),
    'cd_ekf-chirp-n2': (q('cd_ekf', 'chirp_sde1', n=2), 'cdekf4_mfma wave=1 segs=1'),
    'cd_ekf-chirp-n16': (q('cd_ekf', 'chirp_sde1', n=16), 'cdekf4_mfma wave=1 segs=1'),
    'cd_sgp-chirp': (q('cd_sgp', 'chirp_sde1', 'gh3'), 'cdsgp4_mfma wave=1 segs=1'),
    'cd_ekf-chirp-gaps': (q('cd_ekf', 'chirp_sde1', flags=0x2000), 'cdekf4_mfma wave=1 segs=1'),
    'cd_sgp-chirp-gaps': (q('cd_sgp', 'chirp_sde1', 'gh3', flags=0x2000), 'cdsgp4_mfma wave=1 segs=1'),
    'cd_sgp-chirp-ungrouped': (q('cd_sgp', 'chirp_sde1', 'ungrouped'), 'generic_wave wave=1 segs=1'),
    'cd_ekf-chirp-dpp': (q('cd_ekf', 'chirp_sde1', flags=rc.DPP), 'generic_wave wave=1 segs=1'),
    'cd_sgp-chirp-dpp': (q('cd_sgp', 'chirp_sde1', 'gh3', flags=rc.DPP), 'generic_wave wave=1 segs=1'),
    'cd_ekf-chirp-generic': (q('cd_ekf', 'chirp_sde1', flags=rc.GENERIC), 'generic_wave wave=1 segs=1'),
    'cd_ekf-chirp-thread': (q('cd_ekf', 'chirp_sde1', B=70, flags=rc.THREAD), 'generic_lane wave=0 segs=1'),
    'cd_sgp-chirp-thread': (q('cd_sgp', 'chirp_sde1', 'gh3', B=70, flags=rc.THREAD), 'generic_lane wave=0 segs=1'),
    'cd_ekf-harm2': (q('cd_ekf', 'chirp_sde2'), 'generic_wave wave=1 segs=1'),
    'cd_sgp-linear4': (q('cd_sgp', 'linear_sde4', 'gh3'), 'generic_wave wave=1 segs=1'),
    # the generic crossovers on 256 CUs ({5, 2}; sigma-point {8, 1}), not the matrix-core kernels' (4 and 48 trials per SIMD)
    'cd_ekf-chirp-b2559': (q('cd_ekf', 'chirp_sde1', B=2559, T=64), 'cdekf4_mfma wave=1 segs=1'),
    'cd_ekf-chirp-b2560': (q('cd_ekf', 'chirp_sde1', B=2560, T=64), 'generic_lane wave=0 segs=1'),
    'cd_sgp-chirp-b8191': (q('cd_sgp', 'chirp_sde1', 'gh3', B=8191, T=64), 'cdsgp4_mfma wave=1 segs=1'),
    'cd_sgp-chirp-b8192': (q('cd_sgp', 'chirp_sde1', 'gh3', B=8192, T=64), 'generic_lane wave=0 segs=1'),
    # smoothers: the generic kernel with one wavefront per trial whatever the batch, selected outputs gathered from its rows
    'cd_eks-chirp': (q('cd_eks', 'chirp_sde1', entry='smoother'), 'sde_harm' + SMOOTHER_PLAN + 'none'),
    'cd_sgps-chirp': (q('cd_sgp', 'chirp_sde1', 'gh3', entry='smoother'), 'sde_harm' + SMOOTHER_PLAN + 'none'),
    'cd_eks-chirp-dpp': (q('cd_eks', 'chirp_sde1', entry='smoother', flags=rc.DPP), 'sde_harm' + SMOOTHER_PLAN + 'none'),
    'cd_eks-chirp-b40000': (q('cd_eks', 'chirp_sde1', entry='smoother', B=40000, T=64), 'sde_harm' + SMOOTHER_PLAN + 'none'),
    'cd_sgps-chirp-b40000': (q('cd_sgp', 'chirp_sde1', 'gh3', entry='smoother', B=40000, T=64), 'sde_harm' + SMOOTHER_PLAN + 'none'),
    'cd_eks-harm2': (q('cd_eks', 'chirp_sde2', entry='smoother'), 'sde_harm' + SMOOTHER_PLAN + 'none'),
    'cd_eks-linear4': (q('cd_eks', 'linear_sde4', entry='smoother'), 'sde_linear' + SMOOTHER_PLAN + 'none'),
    'cd_eks-chirp-select': (q('cd_eks', 'chirp_sde1', entry='select'), 'sde_harm' + SMOOTHER_PLAN + 'gather'),
    'cd_sgps-chirp-select': (q('cd_sgp', 'chirp_sde1', 'gh3', entry='select'), 'sde_harm' + SMOOTHER_PLAN + 'gather'),
    # refused: what has no kernel for it
    'cd_eks-chirp-select-null': (q('cd_eks', 'chirp_sde1', entry='select', null_rows=True), 'refused: this (method'),
    'cd_eks-chirp-thread': (q('cd_eks', 'chirp_sde1', entry='smoother', B=70, flags=rc.THREAD), 'refused: CGP_RK4_SUBSTEPS'),
    'cd_sgps-chirp-big': (q('cd_sgp', 'chirp_sde1', 'big', entry='smoother'), 'refused: CGP_RK4_SUBSTEPS'),
    'fsplit-cd_sgp': (q('cd_sgp', 'chirp_sde1', 'gh3', T=256, entry='filter_split', segments=2), 'refused: CGP_RK4_SUBSTEPS'),
    'ssplit-cd_eks': (q('cd_eks', 'chirp_sde1', T=256, entry='smoother_split', segments=2), 'refused: CGP_RK4_SUBSTEPS'),
    'ekf-chirp': (q('ekf', 'chirp'), 'refused: CGP_RK4_SUBSTEPS'),
    'sgp-harm3': (q('sgp', 'harm3', 'cub'), 'refused: CGP_RK4_SUBSTEPS'),
    'kpt2': (q('ekf_kpt', 'kpt2'), 'refused: CGP_RK4_SUBSTEPS'),
    'eks-chirp': (q('eks', 'chirp', entry='smoother'), 'refused: CGP_RK4_SUBSTEPS'),
    'rts-linear4': (q('eks', 'linear4', entry='smoother'), 'refused: CGP_RK4_SUBSTEPS'),
}
HONOURING = ('generic_wave', 'generic_lane', 'cdekf4_mfma', 'cdsgp4_mfma', 'sde_harm', 'sde_linear')


def _build(tmp_path_factory, name, extra=()):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path_factory.mktemp(name + '_substeps') / name)
    subprocess.run([hipcc, '--cuda-host-only', *extra, '-O1', '-std=c++17', '-Wno-int-to-pointer-cast', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', name + '.hip'), '-o', exe], check=True)
    return exe


@pytest.fixture(scope='module')
def routed(tmp_path_factory):
    exe = _build(tmp_path_factory, 'route_probe')
    ids = list(ROUTES)
    lines = ''.join(rc.probe_line(ROUTES[i][0]) + '\n' for i in ids)
    out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ids), out
    return dict(zip(ids, out))


@pytest.mark.parametrize('cid', list(ROUTES))
def test_flagged_route(routed, cid):
    want, got = ROUTES[cid][1], routed[cid]
    if want.startswith('refused'):
        assert got.startswith(want), got                  # the message names the flag (or, for a selection without rows, is the existing one)
    else:
        assert got == want, (cid, got, want)
        assert got.split()[0] in HONOURING and (ROUTES[cid][0]['entry'] == 'filter' or ' wave=1 ' in got)


def test_the_pinned_case_list_is_untouched():
    assert not any(c['flags'] & 0x000F0000 for c in rc.CASES)


# ---- the entry points: refusals with their codes (csrc/cgp_args.hpp), through the pure half of each

def _cd_filter(n=4, **kw):
    return ac._both(ac._set(method=ac.F_CD_EKF, model=ac.sde(), flags=SUB(n)), ac._set(**kw))


def _cd_smoother(n=4, **kw):
    return ac._both(ac._set(method=ac.S_CD_EKS, model=ac.sde(), flags=SUB(n)), ac._set(**kw))


ABI = {
    'cgp_filter cd_ekf n = 4': ('cgp_filter', _cd_filter(), 'ok'),
    'cgp_filter cd_ekf n = 16 with gaps': ('cgp_filter', _cd_filter(flags=SUB(16) | ac.SKIP_MISSING), 'ok'),
    'cgp_filter cd_sgp n = 2': ('cgp_filter', ac._set(method=ac.F_CD_SGP, model=ac.sde(), sigma=ac.cubature(), flags=SUB(2)), 'ok'),
    'cgp_filter ekf': ('cgp_filter', ac._set(method=ac.F_EKF, model=ac.lcd(), flags=SUB(2)), f'refused {ac.E_ARG}: CGP_RK4_SUBSTEPS'),
    'cgp_filter sgp': ('cgp_filter', ac._set(method=ac.F_SGP, model=ac.lcd(), sigma=ac.cubature(), flags=SUB(3)), f'refused {ac.E_ARG}: CGP_RK4_SUBSTEPS'),
    'cgp_filter_time_split': ('cgp_filter_time_split', _cd_filter(), f'refused {ac.E_UNSUPPORTED}: CGP_RK4_SUBSTEPS'),
    'cgp_filter_time_split one segment': ('cgp_filter_time_split', _cd_filter(segments=1), f'refused {ac.E_UNSUPPORTED}: CGP_RK4_SUBSTEPS'),
    'cgp_smoother cd_eks n = 4': ('cgp_smoother', _cd_smoother(), 'ok'),
    'cgp_smoother cd_sgp n = 3': ('cgp_smoother', ac._set(method=ac.S_CD_SGP, model=ac.sde(), sigma=ac.cubature(), flags=SUB(3)), 'ok'),
    'cgp_smoother eks': ('cgp_smoother', ac._set(method=ac.S_EKS, model=ac.lcd(), flags=SUB(2)), f'refused {ac.E_ARG}: CGP_RK4_SUBSTEPS'),
    'cgp_smoother cd_eks one lane per trial': ('cgp_smoother', _cd_smoother(flags=SUB(2) | ac.THREAD_PER_TRIAL), f'refused {ac.E_UNSUPPORTED}: CGP_RK4_SUBSTEPS'),
    'cgp_smoother_select cd_eks': ('cgp_smoother_select', _cd_smoother(), 'ok'),
    'cgp_smoother_time_split': ('cgp_smoother_time_split', _cd_smoother(), f'refused {ac.E_UNSUPPORTED}: CGP_RK4_SUBSTEPS'),
    'cgp_smoother_sample': ('cgp_smoother_sample', ac._set(flags=SUB(2)), f'refused {ac.E_ARG}: cgp_smoother_sample takes no flag: bit 0x10000 (CGP_RK4_SUBSTEPS) is set'),
    'cgp_pcrlb_sums': ('cgp_pcrlb_sums', ac._set(flags=SUB(3)), f'refused {ac.E_ARG}: cgp_pcrlb_sums takes no flag: bit 0x20000 (CGP_RK4_SUBSTEPS) is set'),
    'cgp_ekf_nll_grad': ('cgp_ekf_nll_grad', ac._set(flags=SUB(2)), f'refused {ac.E_ARG}: cgp_ekf_nll_grad takes CGP_SKIP_MISSING and no other flag: bit 0x10000 (CGP_RK4_SUBSTEPS) is set'),
    'cgp_sgp_nll_fisher': ('cgp_sgp_nll_fisher', ac._set(flags=SUB(5) | ac.SKIP_MISSING), f'refused {ac.E_ARG}: cgp_sgp_nll_fisher takes CGP_SKIP_MISSING and no other flag: bit 0x40000 (CGP_RK4_SUBSTEPS) is set'),
    'cgp_cd_ekf_nll_grad n = 5 with gaps': ('cgp_cd_ekf_nll_grad', ac._set(flags=SUB(5) | ac.SKIP_MISSING), 'ok'),
    'cgp_cd_ekf_nll_grad n = 16': ('cgp_cd_ekf_nll_grad', ac._set(flags=SUB(16)), 'ok'),
    'cgp_cd_ekf_nll_grad another flag': ('cgp_cd_ekf_nll_grad', ac._set(flags=SUB(2) | ac.WAVE_PER_TRIAL), f'refused {ac.E_ARG}: cgp_cd_ekf_nll_grad takes CGP_SKIP_MISSING and no other flag: bit 0x2 (CGP_WAVE_PER_TRIAL) is set'),
    # run-time compiled models: an SDE model's entry points take the bits, a discrete model's refuse them like a discrete method
    'cgp_filter_custom discrete': ('cgp_filter_custom', ac._set(flags=SUB(2)), f'refused {ac.E_ARG}: CGP_RK4_SUBSTEPS'),
    'cgp_smoother_custom discrete': ('cgp_smoother_custom', ac._set(flags=SUB(2)), f'refused {ac.E_ARG}: CGP_RK4_SUBSTEPS'),
    'cgp_filter_custom sde': ('cgp_filter_custom', ac._both(ac._field('m', kind=1), ac._set(gamma='gamma', flags=SUB(4) | ac.SKIP_MISSING)), 'ok'),
    'cgp_smoother_custom sde': ('cgp_smoother_custom', ac._both(ac._field('m', kind=1), ac._set(gamma='gamma', flags=SUB(16))), 'ok'),
    'cgp_smoother_custom sde, a set too large': ('cgp_smoother_custom', ac._both(ac._field('m', kind=1), ac._set(gamma='gamma', flags=SUB(2), sigma=ac.Rec(s=2000, d=2, xi='xi', w='w', group_start=None, n_groups=0, flags=0))),
                                                 f'refused {ac.E_UNSUPPORTED}: CGP_RK4_SUBSTEPS'),
}


@pytest.fixture(scope='module')
def prepared(tmp_path_factory):
    exe = _build(tmp_path_factory, 'abi_probe', ('-no-hip-rt',))
    ids = list(ABI)
    lines = ''.join(ac.probe_line(ABI[i][0], ac.arguments(ABI[i][0], ABI[i][1])) + '\n' for i in ids)
    out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ids), out
    return dict(zip(ids, out))


@pytest.mark.parametrize('cid', list(ABI))
def test_flagged_entry_point(prepared, cid):
    want, got = ABI[cid][2], prepared[cid]
    assert got.startswith(want) if want.startswith('refused') else got == want, (cid, got)
