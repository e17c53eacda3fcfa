"""`dts=` (include/chirpgp_hip_timed.h) without a GPU: the stepped oracle that defines it (tests/times_oracle.py), the header and its two
symbols, the refusals of both entry points and the kernel each timed call would run -- through a host probe of its own,
tests/timed_probe.hip --, every ValueError of the Python layer, and tools.intervals.

The tests of the header, the symbols, the source hash, the probe's two tables, the Python refusals and tools.intervals fail on the parent
commit: the keyword, the header, the symbols and the probe's members do not exist there.  The three tests of the definition run the oracle
alone and test_the_existing_probes_compile_unchanged pins what must NOT change: those four pass on the parent too."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import np_filters as onp
from oracle import np_models as om
from oracle.np_quadratures import SigmaPoints as OSigmaPoints
from tests import cases as cs
from tests import gap_oracle as go
from tests import route_cases as rc
from tests import substeps_oracle as so
from tests import times_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'chirpgp_hip_timed.h')
E_ARG, E_UNSUPPORTED = -1, -2


def SUB(n):
    return (n - 1) << 16                                  # CGP_RK4_SUBSTEPS(n)


# ---- the definition
def oracle_models():
    """(name, drift, dispersion, m0, P0, H, Xi, dt, ys, cubature set) of the four models of tests/test_gpu_times.py, T = 40."""
    out = []
    for name, c in (('chirp', cs.chirp_case(T=40)), ('lascala', cs.lascala_case(T=40)), ('harm3', cs.harmonic_case(nh=3, T=40)),
                    ('linear3', cs.linear_case(0, T=40))):
        out.append((name, c.o_drift, c.o_disp, c.m0, c.P0, c.H, c.Xi, c.dt, c.ys, OSigmaPoints.cubature(c.d)))
    return out


def test_the_stepped_oracle_on_a_constant_grid_is_the_plain_oracle_bit_for_bit():
    for name, drift, disp, m0, P0, H, Xi, dt, ys, _ in oracle_models():
        plain = onp.cd_ekf(drift, disp, H, Xi, m0, P0, dt, ys)
        timed = to.run_filter(onp.cd_ekf, drift, disp, H, Xi, m0, P0, np.full(ys.size, dt), ys)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(timed, plain)), name
        splain = onp.cd_eks(drift, disp, plain[0], plain[1], dt)
        stimed = to.run_smoother(onp.cd_eks, drift, disp, plain[0], plain[1], np.full(ys.size, dt))
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(stimed, splain)), name
    # ... and the sigma-point pair on the chirp
    name, drift, disp, m0, P0, H, Xi, dt, ys, sg = oracle_models()[0]
    plain = onp.cd_sgp_filter(drift, disp(None), sg, H, Xi, m0, P0, dt, ys)
    timed = to.run_filter(onp.cd_sgp_filter, drift, disp(None), sg, H, Xi, m0, P0, np.full(ys.size, dt), ys)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(timed, plain))
    splain = onp.cd_sgp_smoother(drift, disp(None), sg, plain[0], plain[1], dt)
    stimed = to.run_smoother(onp.cd_sgp_smoother, drift, disp(None), sg, plain[0], plain[1], np.full(ys.size, dt))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(stimed, splain))


def test_the_grids_of_the_gpu_tests_keep_all_four_oracle_methods_finite():
    """dt (1 + 0.75 u) with one interval of 3 dt and one of zero on the chirp, La Scala and three-harmonic models; dt (1 + 0.25 u) with a
    zero interval on the linear SDE, whose cd_sgp_smoother oracle leaves the reals from 1.5 dt on."""
    for name, drift, disp, m0, P0, H, Xi, dt, ys, sg in oracle_models():
        dts = to.grid(ys.size, dt, 0.25, zero_at=30) if name == 'linear3' else to.grid(ys.size, dt, 0.75, long_at=20, zero_at=30)
        assert dts.min() == 0.0 and (name == 'linear3' or dts.max() == 3 * dt)
        f = to.run_filter(onp.cd_ekf, drift, disp, H, Xi, m0, P0, dts, ys)
        s = to.run_smoother(onp.cd_eks, drift, disp, f[0], f[1], dts)
        fs_ = to.run_filter(onp.cd_sgp_filter, drift, disp(None), sg, H, Xi, m0, P0, dts, ys)
        ss = to.run_smoother(onp.cd_sgp_smoother, drift, disp(None), sg, fs_[0], fs_[1], dts)
        assert all(np.isfinite(a).all() for a in f + s + fs_ + ss), name
        # a zero interval is the identity: the prediction of step 30 is the filtering result of step 29, so its update is the oracle's own
        # update of that row with the second sample
        upd = onp._linear_update(f[0][29], f[1][29], H, Xi, ys[30])
        assert np.array_equal(f[0][30], upd[0]) and np.array_equal(f[1][30], upd[1]), name
        # and the smoother does not read dts[0]
        other = dts.copy()
        other[0] = 123.0
        assert all(np.array_equal(a, b) for a, b in zip(to.run_smoother(onp.cd_eks, drift, disp, f[0], f[1], other), s))


def test_timed_substeps_are_the_refined_timed_record_bit_for_bit():
    """Timed + substeps is the timed oracle on the refined record -- NaN at the inserted times, under the gap rule -- over dts[t] / n
    repeated n times; n = 1 is the timed oracle itself, and a NaN of the caller's record is a gap like the inserted ones."""
    name, drift, disp, m0, P0, H, Xi, dt, ys, sg = oracle_models()[0]
    dts = to.grid(ys.size, dt, 0.75, long_at=20, zero_at=30)
    one, full = to.run_filter_substeps(onp.cd_ekf, 1, drift, disp, H, Xi, m0, P0, dts, ys)
    plain = to.run_filter(onp.cd_ekf, drift, disp, H, Xi, m0, P0, dts, ys)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(one, plain, full))
    for n in (2, 3):
        fine, ref = to.refine_grid(dts, n), so.refine(ys, n)
        assert fine.shape == (n * ys.size,) and np.array_equal(fine[::n], dts / n) and np.array_equal(fine[n - 1::n], dts / n)
        kept, full = to.run_filter_substeps(onp.cd_ekf, n, drift, disp, H, Xi, m0, P0, dts, ys)
        want = to.run_filter(onp.cd_ekf, drift, disp, H, Xi, m0, P0, fine, ref, skip=True)
        assert all(np.array_equal(a, b) for a, b in zip(full, want)) and all(np.array_equal(a, b[so.kept(n)]) for a, b in zip(kept, want))
        assert np.isfinite(kept[0]).all() and not np.array_equal(kept[0], plain[0])
        sm = to.run_smoother_substeps(onp.cd_eks, n, drift, disp, full[0], full[1], dts)
        want_s = to.run_smoother(onp.cd_eks, drift, disp, full[0], full[1], fine)
        assert all(np.array_equal(a, b[so.kept(n)]) for a, b in zip(sm, want_s)) and np.isfinite(sm[0]).all()
    # on a constant grid the refined timed record is tests/substeps_oracle.py's
    kept, _ = to.run_filter_substeps(onp.cd_ekf, 2, drift, disp, H, Xi, m0, P0, np.full(ys.size, dt), ys)
    want, _ = so.run_filter(onp.cd_ekf, 2, drift, disp, H, Xi, m0, P0, dt, ys)
    assert all(np.array_equal(a, b) for a, b in zip(kept, want))
    gapped = go.with_gaps(ys, ((3, 5), (39, 40)))
    kept, _ = to.run_filter_substeps(onp.cd_ekf, 2, drift, disp, H, Xi, m0, P0, dts, gapped)
    assert np.isfinite(kept[0]).all() and kept[2][3] == kept[2][2] == kept[2][4]      # the NLL holds over the gap


# ---- the header, its symbols, the source hash
def _declared(path):
    src = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(cgp_[a-z0-9_]+)\s*\(', src)))


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from chirpgp_amd import _engine
    return _engine.load_library(), _engine


def test_timed_exports_are_the_headers_symbols_and_the_first_header_is_untouched():
    lib, eng = _lib()
    assert _declared(HEADER) == sorted(eng.TIMED_EXPORTS) == ['cgp_filter_timed', 'cgp_smoother_timed']
    for n in eng.TIMED_EXPORTS:
        assert hasattr(lib, n), f'{n} declared in chirpgp_hip_timed.h but not exported'
    first = _declared(os.path.join(ROOT, 'include', 'chirpgp_hip.h'))
    assert set(first) == set(eng.EXPORTS) and not set(eng.EXPORTS) & set(eng.TIMED_EXPORTS)
    assert lib.cgp_version() == 160                       # CGP_VERSION stays: the new symbols have a version of their own
    src = open(HEADER).read()
    assert re.search(r'#define\s+CGP_TIMED_VERSION\s+1\b', src) and eng.TIMED_VERSION == 1
    assert '#include "chirpgp_hip.h"' in src
    # the null context is refused without a GPU, like cgp_filter's
    assert lib.cgp_filter_timed(None, 2, None, None, None, None, 0, None, 1, 1, None, 1, 1, None, None, None, 0, None) == E_ARG
    assert lib.cgp_smoother_timed(None, 2, None, None, None, 0, 1, None, None, None, 1, 1, None, 0, None) == E_ARG


def test_the_source_hash_covers_the_new_header():
    lib, eng = _lib()
    assert lib.cgp_source_hash().decode() == eng.source_hash()
    make = open(os.path.join(ROOT, 'chirpgp_amd', 'csrc', 'Makefile')).read()
    line = re.search(r'^HASH_SRCS\s*=(.*)$', make, flags=re.M).group(1)
    assert line.split()[-2:] == ['../../include/chirpgp_hip.h', '../../include/chirpgp_hip_timed.h']
    import hashlib
    import glob
    src = os.path.join(ROOT, 'chirpgp_amd', 'csrc')
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(src, '*.hip')) + glob.glob(os.path.join(src, '*.hpp')))
    h = hashlib.sha256()
    for f in [os.path.join(src, n) for n in names] + [os.path.join(src, 'Makefile'), os.path.join(ROOT, 'include', 'chirpgp_hip.h'), HEADER]:
        h.update(open(f, 'rb').read())
    assert h.hexdigest() == eng.source_hash()


def test_both_headers_are_plain_c_and_a_c_program_links_against_the_library(tmp_path):
    if not shutil.which('gcc'):
        pytest.skip('no gcc')
    _lib()
    src = tmp_path / 'timed.c'
    src.write_text('#include <stdio.h>\n#include "chirpgp_hip.h"\n#include "chirpgp_hip_timed.h"\n'
                   'int main(void) {\n'
                   '    cgp_smooth_out out;\n'
                   '    out.mss = NULL;\n'
                   '    printf("%d %d\\n", cgp_version(), CGP_TIMED_VERSION);\n'
                   '    return cgp_filter_timed(NULL, CGP_F_CD_EKF, NULL, NULL, NULL, NULL, 0, NULL, 1, 1, NULL, 1, 1, NULL, NULL, NULL, 0u, NULL) == CGP_E_ARG\n'
                   '        && cgp_smoother_timed(NULL, CGP_S_CD_EKS, NULL, NULL, NULL, 0, 1, NULL, NULL, NULL, 1, 1, &out, CGP_RK4_SUBSTEPS(2), NULL) == CGP_E_ARG ? 0 : 1;\n}\n')
    inc, libdir = os.path.join(ROOT, 'include'), os.path.join(ROOT, 'chirpgp_amd')
    exe = tmp_path / 'timed'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', f'-I{inc}', str(src), '-o', str(exe), f'-L{libdir}', '-lchirpgp_hip',
                    f'-Wl,-rpath,{libdir}', '-Wl,-rpath,/opt/rocm/lib'], check=True, capture_output=True)
    subprocess.run(['g++', '-std=c++11', '-Wall', '-Wextra', '-Werror', f'-I{inc}', '-x', 'c++', '-fsyntax-only', str(src)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [160, 1], out
    assert ctypes.sizeof(ctypes.c_double) == 8


# ---- the probe: refusals of both entry points, and the kernel each timed call would run
MODELS = dict(rc.MODELS)
MODELS.update({'chirp_sde3': (4, 8, 3, 'sde'), 'linear_sde3': (3, 3, 0, 'sde'), 'linear_sde8': (3, 8, 0, 'sde')})
N_PARAMS = {0: lambda d: 2 * d * d, 1: lambda d: 5, 2: lambda d: 2, 3: lambda d: d * d, 4: lambda d: 3, 5: lambda d: 2 * d * d}


def sigma_shape(kind, model):
    if kind is None:
        return (0, 0, 0, 0)
    model_id, d = MODELS[model][0], MODELS[model][1]
    if model in rc.MODELS:
        s, n_groups, grouped, flags = rc.sigma_shape(kind, model)
    else:
        grouped = model_id in rc.NONLINEAR
        s, n_groups, flags = (2 * d, 2 * d - 1, rc.SIGMA_STANDARD | rc.SIGMA_AXIAL) if grouped else (2 * d, 0, 0)
    return (s, n_groups, int(grouped), flags)


def q(method, model, sigma=None, B=4, T=128, flags=0, entry='filter', dts=1, dts_stride=0, dts_repeat=1, null_rows=False, num_cus=256):
    table = rc.FILTERS if entry == 'filter' else rc.SMOOTHERS
    model_id, d, n_harm, _ = MODELS[model]
    return ' '.join(str(v) for v in (entry, table[method], model_id, d, n_harm, N_PARAMS[model_id](d), *sigma_shape(sigma, model), B, T, flags, dts,
                                     dts_stride, dts_repeat, int(null_rows), num_cus))


F = ' timed=1 sub=0 gaps=0 stride=0'
S = ' timed=1 sub=0 sel='
ROUTES = {
    # filters: the d = 4 matrix-core kernel where the untimed call with the same flags runs it one wavefront per trial ...
    'cd_ekf-chirp': (q('cd_ekf', 'chirp_sde1'), 'cdekf4_mfma wave=1' + F),
    'cd_sgp-chirp': (q('cd_sgp', 'chirp_sde1', 'gh3'), 'cdsgp4_mfma wave=1' + F),
    'cd_sgp-chirp-cub': (q('cd_sgp', 'chirp_sde1', 'cub'), 'cdsgp4_mfma wave=1' + F),
    'cd_ekf-chirp-own-grids': (q('cd_ekf', 'chirp_sde1', dts_stride=128), 'cdekf4_mfma wave=1 timed=1 sub=0 gaps=0 stride=128'),
    'cd_ekf-chirp-odd-stride': (q('cd_ekf', 'chirp_sde1', dts_stride=1000), 'cdekf4_mfma wave=1 timed=1 sub=0 gaps=0 stride=1000'),
    'cd_ekf-chirp-gaps': (q('cd_ekf', 'chirp_sde1', flags=0x2000), 'cdekf4_mfma wave=1 timed=1 sub=0 gaps=1 stride=0'),
    'cd_sgp-chirp-gaps': (q('cd_sgp', 'chirp_sde1', 'gh3', flags=0x2000), 'cdsgp4_mfma wave=1 timed=1 sub=0 gaps=1 stride=0'),
    'cd_ekf-chirp-n4': (q('cd_ekf', 'chirp_sde1', flags=SUB(4)), 'cdekf4_mfma wave=1 timed=1 sub=1 gaps=0 stride=0'),
    'cd_sgp-chirp-n16-gaps': (q('cd_sgp', 'chirp_sde1', 'gh3', flags=SUB(16) | 0x2000), 'cdsgp4_mfma wave=1 timed=1 sub=1 gaps=1 stride=0'),
    'cd_ekf-chirp-final-nll': (q('cd_ekf', 'chirp_sde1', flags=0x1), 'cdekf4_mfma wave=1' + F),
    # ... with the untimed call's crossovers: cd_ekf 4 trials per SIMD on 256 CUs, cd_sgp 48; flagged calls the generic limits
    'cd_ekf-chirp-b4095': (q('cd_ekf', 'chirp_sde1', B=4095, T=64), 'cdekf4_mfma wave=1' + F),
    'cd_ekf-chirp-b4096': (q('cd_ekf', 'chirp_sde1', B=4096, T=64), 'generic_lane wave=0' + F),
    'cd_sgp-chirp-b49151': (q('cd_sgp', 'chirp_sde1', 'gh3', B=49151, T=64), 'cdsgp4_mfma wave=1' + F),
    'cd_sgp-chirp-b49152': (q('cd_sgp', 'chirp_sde1', 'gh3', B=49152, T=64), 'generic_lane wave=0' + F),
    'cd_ekf-chirp-n4-b2559': (q('cd_ekf', 'chirp_sde1', B=2559, T=64, flags=SUB(4)), 'cdekf4_mfma wave=1 timed=1 sub=1 gaps=0 stride=0'),
    'cd_ekf-chirp-n4-b2560': (q('cd_ekf', 'chirp_sde1', B=2560, T=64, flags=SUB(4)), 'generic_lane wave=0 timed=1 sub=1 gaps=0 stride=0'),
    # ... and everywhere else the generic kernel in the shape the call has: the DPP forms, the forced shapes, other sets, other models
    'cd_ekf-chirp-dpp': (q('cd_ekf', 'chirp_sde1', flags=rc.DPP), 'generic_wave wave=1' + F),
    'cd_sgp-chirp-dpp': (q('cd_sgp', 'chirp_sde1', 'gh3', flags=rc.DPP), 'generic_wave wave=1' + F),
    'cd_ekf-chirp-generic': (q('cd_ekf', 'chirp_sde1', flags=rc.GENERIC), 'generic_wave wave=1' + F),
    'cd_ekf-chirp-thread': (q('cd_ekf', 'chirp_sde1', B=70, flags=rc.THREAD), 'generic_lane wave=0' + F),
    'cd_sgp-chirp-thread': (q('cd_sgp', 'chirp_sde1', 'gh3', B=70, flags=rc.THREAD), 'generic_lane wave=0' + F),
    'cd_ekf-chirp-wave-b40000': (q('cd_ekf', 'chirp_sde1', B=40000, T=64, flags=rc.WAVE), 'cdekf4_mfma wave=1' + F),
    'cd_sgp-chirp-ungrouped': (q('cd_sgp', 'chirp_sde1', 'ungrouped'), 'generic_wave wave=1' + F),      # (untimed: the DPP form, which knows no intervals)
    'cd_sgp-chirp-big': (q('cd_sgp', 'chirp_sde1', 'big'), 'generic_lane wave=0' + F),
    'cd_ekf-harm2': (q('cd_ekf', 'chirp_sde2'), 'generic_wave wave=1' + F),
    'cd_sgp-harm3': (q('cd_sgp', 'chirp_sde3', 'cub'), 'generic_wave wave=1' + F),
    'cd_ekf-harm3-thread': (q('cd_ekf', 'chirp_sde3', B=70, flags=rc.THREAD), 'generic_lane wave=0' + F),
    'cd_ekf-linear4': (q('cd_ekf', 'linear_sde4'), 'generic_wave wave=1' + F),
    'cd_sgp-linear3-n2': (q('cd_sgp', 'linear_sde3', 'cub', flags=SUB(2)), 'generic_wave wave=1 timed=1 sub=1 gaps=0 stride=0'),
    'cd_ekf-linear8': (q('cd_ekf', 'linear_sde8'), 'generic_wave wave=1' + F),
    # smoothers: the matrix-core walks one wavefront per trial, else the generic kernel in the shape the call has
    'cd_eks-chirp': (q('cd_eks', 'chirp_sde1', entry='smoother'), 'cdeks4_mfma wave=1' + S + 'none stride=0 repeat=1'),
    'cd_sgps-chirp': (q('cd_sgp', 'chirp_sde1', 'gh3', entry='smoother'), 'cdsgps4_mfma wave=1' + S + 'none stride=0 repeat=1'),
    'cd_eks-chirp-addressed': (q('cd_eks', 'chirp_sde1', entry='smoother', dts_stride=128, dts_repeat=13), 'cdeks4_mfma wave=1' + S + 'none stride=128 repeat=13'),
    'cd_eks-chirp-dpp': (q('cd_eks', 'chirp_sde1', entry='smoother', flags=rc.DPP), 'sde_harm wave=1' + S + 'none stride=0 repeat=1'),
    'cd_sgps-chirp-dpp': (q('cd_sgp', 'chirp_sde1', 'gh3', entry='smoother', flags=rc.DPP), 'sde_harm wave=1' + S + 'none stride=0 repeat=1'),
    'cd_eks-chirp-generic': (q('cd_eks', 'chirp_sde1', entry='smoother', flags=rc.GENERIC), 'sde_harm wave=1' + S + 'none stride=0 repeat=1'),
    'cd_eks-chirp-thread': (q('cd_eks', 'chirp_sde1', entry='smoother', B=70, flags=rc.THREAD), 'sde_harm wave=0' + S + 'none stride=0 repeat=1'),
    'cd_eks-chirp-b3071': (q('cd_eks', 'chirp_sde1', entry='smoother', B=3071, T=64), 'cdeks4_mfma wave=1' + S + 'none stride=0 repeat=1'),
    'cd_eks-chirp-b3072': (q('cd_eks', 'chirp_sde1', entry='smoother', B=3072, T=64), 'sde_harm wave=0' + S + 'none stride=0 repeat=1'),
    'cd_sgps-chirp-b49152': (q('cd_sgp', 'chirp_sde1', 'gh3', entry='smoother', B=49152, T=64), 'sde_harm wave=0' + S + 'none stride=0 repeat=1'),
    'cd_eks-harm2': (q('cd_eks', 'chirp_sde2', entry='smoother'), 'sde_harm wave=1' + S + 'none stride=0 repeat=1'),
    'cd_sgps-harm3': (q('cd_sgp', 'chirp_sde3', 'cub', entry='smoother'), 'sde_harm wave=1' + S + 'none stride=0 repeat=1'),
    'cd_eks-linear4': (q('cd_eks', 'linear_sde4', entry='smoother'), 'sde_linear wave=1' + S + 'none stride=0 repeat=1'),
    'cd_eks-linear4-thread': (q('cd_eks', 'linear_sde4', entry='smoother', B=70, flags=rc.THREAD), 'sde_linear wave=0' + S + 'none stride=0 repeat=1'),
    # ... with substeps the generic wave kernel, as untimed
    'cd_eks-chirp-n4': (q('cd_eks', 'chirp_sde1', entry='smoother', flags=SUB(4)), 'sde_harm wave=1 timed=1 sub=1 sel=none stride=0 repeat=1'),
    'cd_sgps-chirp-n2-b40000': (q('cd_sgp', 'chirp_sde1', 'gh3', entry='smoother', B=40000, T=64, flags=SUB(2)), 'sde_harm wave=1 timed=1 sub=1 sel=none stride=0 repeat=1'),
    # ... and selected outputs gathered from the full rows
    'cd_eks-chirp-select': (q('cd_eks', 'chirp_sde1', entry='select'), 'cdeks4_mfma wave=1' + S + 'gather stride=0 repeat=1'),
    'cd_eks-chirp-select-thread': (q('cd_eks', 'chirp_sde1', entry='select', B=70, flags=rc.THREAD), 'sde_harm wave=0' + S + 'gather stride=0 repeat=1'),
}
REFUSALS = {
    # the rows of the header
    'filter dts NULL': (q('cd_ekf', 'chirp_sde1', dts=0), f'refused {E_ARG}: dts is NULL'),
    'filter dts_stride < 0': (q('cd_ekf', 'chirp_sde1', dts_stride=-1), f'refused {E_ARG}: dts_stride must be >= 0'),
    'smoother dts NULL': (q('cd_eks', 'chirp_sde1', entry='smoother', dts=0), f'refused {E_ARG}: dts is NULL'),
    'smoother dts_stride < 0': (q('cd_eks', 'chirp_sde1', entry='smoother', dts_stride=-128), f'refused {E_ARG}: dts_stride must be >= 0'),
    'smoother dts_repeat < 1': (q('cd_eks', 'chirp_sde1', entry='smoother', dts_repeat=0), f'refused {E_ARG}: dts_repeat must be >= 1'),
    'select dts_repeat < 1': (q('cd_sgp', 'chirp_sde1', 'gh3', entry='select', dts_repeat=-3), f'refused {E_ARG}: dts_repeat must be >= 1'),
    # discrete methods and models: their constants are fixed per dt at set-up
    'filter ekf': (q('ekf', 'chirp'), f'refused {E_ARG}: per-step intervals go with the continuous-discrete methods'),
    'filter sgp': (q('sgp', 'harm3', 'cub'), f'refused {E_ARG}: per-step intervals go with the continuous-discrete methods'),
    'filter kf': (q('ekf', 'linear4'), f'refused {E_ARG}: per-step intervals go with the continuous-discrete methods'),
    'filter kpt': (q('ekf_kpt', 'kpt2'), f'refused {E_ARG}: per-step intervals go with the continuous-discrete methods'),
    'filter cd_ekf on a discrete model': (q('cd_ekf', 'chirp'), f'refused {E_ARG}: per-step intervals go with the continuous-discrete methods'),
    'smoother eks': (q('eks', 'chirp', entry='smoother'), f'refused {E_ARG}: per-step intervals go with the continuous-discrete methods'),
    'smoother rts': (q('eks', 'linear4', entry='smoother'), f'refused {E_ARG}: per-step intervals go with the continuous-discrete methods'),
    'smoother sgp': (q('sgp', 'lascala', 'gh3', entry='smoother'), f'refused {E_ARG}: per-step intervals go with the continuous-discrete methods'),
    'smoother cd_sgp on a discrete model': (q('cd_sgp', 'chirp', 'gh3', entry='smoother'), f'refused {E_ARG}: per-step intervals go with the continuous-discrete methods'),
    # the flags' own refusals, as on the plain entry points
    'smoother substeps one lane per trial': (q('cd_eks', 'chirp_sde1', entry='smoother', B=70, flags=SUB(2) | rc.THREAD), f'refused {E_UNSUPPORTED}: CGP_RK4_SUBSTEPS'),
    'smoother substeps, a set too large': (q('cd_sgp', 'chirp_sde1', 'big', entry='smoother', flags=SUB(2)), f'refused {E_UNSUPPORTED}: CGP_RK4_SUBSTEPS'),
    'select without rows': (q('cd_eks', 'chirp_sde1', entry='select', null_rows=True), f'refused {E_UNSUPPORTED}: this (method'),
    'smoother without rows': (q('cd_eks', 'chirp_sde1', entry='smoother', null_rows=True), f'refused {E_ARG}: mfs / Pfs / mss / Pss must be set'),
    'filter negative B': (q('cd_ekf', 'chirp_sde1', B=-1), f'refused {E_ARG}: negative B or T'),
    # empty calls: CGP_OK, nothing touched -- decided before dts is looked at, as before ys
    'filter B = 0': (q('cd_ekf', 'chirp_sde1', B=0), 'empty'),
    'filter T = 0, dts NULL': (q('cd_ekf', 'chirp_sde1', T=0, dts=0), 'empty'),
    'smoother B = 0': (q('cd_eks', 'chirp_sde1', entry='smoother', B=0, dts_repeat=0), 'empty'),
    'smoother T = 0': (q('cd_sgp', 'chirp_sde1', 'gh3', entry='smoother', T=0), 'empty'),
}
HONOURING = ('generic_wave', 'generic_lane', 'cdekf4_mfma', 'cdsgp4_mfma', 'sde_harm', 'sde_linear', 'cdeks4_mfma', 'cdsgps4_mfma')


@pytest.fixture(scope='module')
def probed(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path_factory.mktemp('timed_probe') / 'timed_probe')
    subprocess.run([hipcc, '--cuda-host-only', '-no-hip-rt', '-O1', '-std=c++17', '-Wno-int-to-pointer-cast', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'timed_probe.hip'), '-o', exe], check=True)
    cases = {**ROUTES, **REFUSALS}
    ids = list(cases)
    out = subprocess.run([exe], input=''.join(cases[i][0] + '\n' for i in ids), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ids), out
    return dict(zip(ids, out))


@pytest.mark.parametrize('cid', list(ROUTES))
def test_timed_route(probed, cid):
    want, got = ROUTES[cid][1], probed[cid]
    assert got == want, (cid, got, want)
    assert got.split()[0] in HONOURING and ' timed=1 ' in got


@pytest.mark.parametrize('cid', list(REFUSALS))
def test_timed_refusal(probed, cid):
    want, got = REFUSALS[cid][1], probed[cid]
    assert got.startswith(want) if want.startswith('refused') else got == want, (cid, got)
    if 'per-step intervals' in want:
        assert 'fixed per dt at set-up' in got            # the message says why


def test_the_existing_probes_compile_unchanged(tmp_path):
    """tests/abi_probe.hip and tests/route_probe.hip fill FilterCall / SmootherCall / FilterQuery / SmootherQuery by position: the new members
    trail the old ones with defaults, and an untimed query reaches the decision it reached."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    for name, extra in (('route_probe', ()), ('abi_probe', ('-no-hip-rt',))):
        subprocess.run([hipcc, '--cuda-host-only', *extra, '-O1', '-std=c++17', '-Wno-int-to-pointer-cast', '-fsyntax-only', '-I', os.path.join(ROOT, 'include'),
                        os.path.join(ROOT, 'tests', name + '.hip')], check=True)


# ---- the Python layer: every ValueError, before anything is built or launched
def test_python_refuses_before_anything_is_launched():
    from chirpgp_amd import _engine as E
    from chirpgp_amd import filters_smoothers as fs
    from chirpgp_amd import models as pm
    z, T = np.zeros(4), 5
    ys, dts = np.zeros(T), np.full(T, 1e-3)
    drift, disp, disc, m0, P0, H = pm.build_chirp_model(np.array([0.1, 0.1, 0.1, 1., 1., 7.]))
    mf, Pf = np.zeros((T, 4)), np.stack([np.eye(4)] * T)
    sg = fs.SigmaPoints.cubature(4)
    # both dt and dts
    with pytest.raises(ValueError, match='either dt or dts'):
        fs.cd_ekf(drift, disp, H, 0.1, m0, P0, 1e-3, ys, dts=dts)
    with pytest.raises(ValueError, match='either dt or dts'):
        fs.cd_sgp_smoother(drift, disp, sg, mf, Pf, 1e-3, dts=dts)
    # bad entries, the first one named
    for bad, where in ((np.array([1e-3, np.nan, -1., 1e-3, 1e-3]), r'dts\[1\]'), (np.array([1e-3, 1e-3, -1e-9, np.inf, 1e-3]), r'dts\[2\]'),
                       (np.array([1e-3, 1e-3, 1e-3, -np.inf, np.nan]), r'dts\[3\]')):
        with pytest.raises(ValueError, match=where):
            fs.cd_ekf(drift, disp, H, 0.1, m0, P0, None, ys, dts=bad)
        with pytest.raises(ValueError, match=where):
            fs.cd_eks(drift, disp, mf, Pf, None, dts=bad)
        with pytest.raises(ValueError, match=where):
            fs.cd_sgp_filter(drift, disp, sg, H, 0.1, m0, P0, None, ys, dts=bad)
    two = np.full((2, T), 1e-3)
    two[1, 4] = np.nan
    with pytest.raises(ValueError, match=r'dts\[1, 4\]'):
        fs.cd_ekf(drift, disp, H, 0.1, m0, P0, None, np.zeros((2, T)), dts=two)
    # shapes
    with pytest.raises(ValueError, match='T = 5'):
        fs.cd_ekf(drift, disp, H, 0.1, m0, P0, None, ys, dts=np.full(T + 1, 1e-3))
    with pytest.raises(ValueError, match='time grids'):
        fs.cd_ekf(drift, disp, H, 0.1, m0, P0, None, np.zeros((3, T)), dts=np.full((2, T), 1e-3))
    with pytest.raises(ValueError, match='trials'):
        fs.cd_eks(drift, disp, np.zeros((3, T, 4)), np.zeros((3, T, 4, 4)), None, dts=np.full((2, T), 1e-3))
    # discrete methods
    for call in (lambda: fs.ekf(disc, H, 0.1, m0, P0, None, ys, dts=dts), lambda: fs.eks(disc, mf, Pf, None, dts=dts),
                 lambda: fs.sgp_filter(disc, sg, H, 0.1, m0, P0, None, ys, dts=dts), lambda: fs.sgp_smoother(disc, sg, mf, Pf, None, dts=dts),
                 lambda: fs.kf(np.eye(4), np.eye(4), H, 0.1, m0, P0, ys, dts=dts), lambda: fs.rts(np.eye(4), np.eye(4), mf, Pf, dts=dts),
                 lambda: E.run_filter(E.F_EKF, None, None, None, z, 0.1, z, np.eye(4), None, ys, dts=dts),
                 lambda: E.run_smoother(E.S_SGP, None, None, None, None, mf, Pf, dts=dts)):
        with pytest.raises(ValueError, match='continuous-discrete'):
            call()
    # a run-time compiled drift, a time split: the timed form is not built
    sde, sdisp = pm.custom_sde('dx[0] = -p[0] * x[0];', 1, np.array([1.]), np.eye(1))
    with pytest.raises(ValueError, match='not built'):
        fs.cd_ekf(sde, sdisp, np.ones(1), 0.1, np.zeros(1), np.eye(1), None, ys, dts=dts)
    with pytest.raises(ValueError, match='not built'):
        fs.cd_eks(sde, sdisp, np.zeros((T, 1)), np.ones((T, 1, 1)), None, dts=dts)
    with pytest.raises(ValueError, match='time_split'):
        fs.cd_sgp_filter(drift, disp, sg, H, 0.1, m0, P0, None, ys, dts=dts, time_split=(2, 64))
    with pytest.raises(ValueError, match='time_split'):
        fs.cd_eks(drift, disp, mf, Pf, None, dts=dts, time_split=(2, 64))
    # the grids' addressing without grids
    with pytest.raises(ValueError, match='dts='):
        fs.cd_eks(drift, disp, mf, Pf, 1e-3, trials_per_record=2)


def test_mle_refuses_before_anything_is_built():
    from chirpgp_amd import mle

    def build(*a, **k):
        raise AssertionError('the builder was called')
    th, ys, dts = np.zeros((1, 6)), np.zeros(8), np.full(8, 1e-3)
    for method in ('ekf', 'sgp_filter', 'ekf_for_kpt'):
        for call in (lambda: mle.batched_nll(method, build, th, ys, 0.1, None, dts=dts), lambda: mle.fit(method, build, [1.] * 6, ys, 0.1, None, dts=dts),
                     lambda: mle.fit_many(method, build, [1.] * 6, ys, 0.1, None, dts=dts), lambda: mle.grid_search(method, build, np.ones((2, 6)), ys, 0.1, None, dts=dts),
                     lambda: mle.make_objective(method, build, ys, 0.1, None, dts=dts)):
            with pytest.raises(ValueError, match='dts='):
                call()
    for method in ('cd_ekf', 'cd_sgp_filter'):
        with pytest.raises(ValueError, match='either dt or dts'):
            mle.batched_nll(method, build, th, ys, 0.1, 1e-3, dts=dts)
        with pytest.raises(ValueError, match='tangent kernels take one dt'):
            mle.make_objective(method, build, ys, 0.1, None, exact=True, dts=dts)
        with pytest.raises(ValueError, match='tangent kernels take one dt'):
            mle.fit(method, build, [1.] * 6, ys, 0.1, None, exact=True, dts=dts)
        with pytest.raises(ValueError, match='tangent kernels take one dt'):
            mle.fit_many(method, build, [1.] * 6, ys, 0.1, None, exact=True, dts=dts)
        assert callable(mle.make_objective(method, build, ys, 0.1, None, dts=dts))      # exact=None resolves to the differences: nothing is built yet
    bad = dts.copy()
    bad[3] = -1.0
    with pytest.raises(ValueError, match=r'dts\[3\]'):
        mle.fit_many('cd_ekf', build, [1.] * 6, ys, 0.1, None, dts=bad)


# ---- tools.intervals
def test_intervals():
    from chirpgp_amd import tools
    ts = np.array([0.5, 0.75, 0.75, 1.5])
    assert np.array_equal(tools.intervals(ts), [0.25, 0.25, 0.0, 0.75])                  # t0 defaults to ts[0] - (ts[1] - ts[0])
    assert np.array_equal(tools.intervals(ts, t0=0.0), [0.5, 0.25, 0.0, 0.75])
    assert np.array_equal(tools.intervals(ts, t0=0.5), [0.0, 0.25, 0.0, 0.75])
    grid = 1e-3 * np.arange(1, 101)
    assert np.allclose(tools.intervals(grid), 1e-3, rtol=0, atol=1e-16) and np.array_equal(np.cumsum(tools.intervals(grid, t0=0.0)), np.cumsum(np.diff(grid, prepend=0.0)))
    two = tools.intervals(np.array([[1., 2., 4.], [0., 0.5, 0.5]]), t0=[0.5, -1.0])
    assert np.array_equal(two, [[0.5, 1., 2.], [1., 0.5, 0.]])
    assert np.array_equal(tools.intervals(np.array([[1., 2., 4.], [0., 0.5, 0.5]])), [[1., 1., 2.], [0.5, 0.5, 0.]])
    assert np.array_equal(tools.intervals([2.0], t0=1.5), [0.5])
    for bad, where in (([0.1, 0.3, 0.2], r'ts\[2\]'), ([0.1, np.nan, 0.2], r'ts\[1\]'), ([[0., 1.], [1., 0.5]], r'ts\[1, 1\]')):
        with pytest.raises(ValueError, match=where):
            tools.intervals(bad, t0=-1.0)
    with pytest.raises(ValueError, match=r'ts\[0\]'):
        tools.intervals([0.1, 0.2], t0=0.15)
    with pytest.raises(ValueError, match='t0'):
        tools.intervals([0.1])
    with pytest.raises(ValueError):
        tools.intervals(np.zeros((2, 2, 2)))
    # what the filters take: finite and >= 0
    from chirpgp_amd import _engine as E
    assert E.check_intervals(tools.intervals(ts), 4).shape == (1, 4)
