"""Which kernel a cgp_filter / cgp_smoother launch takes is pinned: the library's route functions (csrc/cgp_route.hpp), asked through the
host program tests/route_probe.hip, answer every case of tests/route_cases.py as tests/golden/routes.json records it.

A smoother's line is its whole launch plan: behind the route and the shape the segments of the exact split and their tiles, the
segments of the split with burn-in, and how selected outputs get written; a refusal is the library's own message.

The golden file: per case the route, and for the cases a 256-CU GPU replays cheaply the kernels the commit BEFORE the route functions
existed launched (one kernel-trace run of the case list on an MI355X); the others ("derived": another CU count, records of gigabytes, a
constructed sigma-point set) have their route read off that commit's dispatch code.  KERNELS ties each route name to the kernel names
of that trace.  No GPU is needed here."""
import json
import os
import re
import shutil
import subprocess

import pytest

from tests import route_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'routes.json')

# route name -> pattern of the kernel it launches, or (with one wavefront per trial, with one lane per trial)
KERNELS = {
    'generic_wave': r'cgp::filter_kernel<cgp::\w+Predict<cgp::(?!Kpt)\w+<\d+>, true',
    'generic_lane': r'cgp::filter_kernel<cgp::\w+Predict<cgp::(?!Kpt)\w+<\d+>, false',
    'generic_kpt': (r'cgp::filter_kernel<cgp::EkfPredict<cgp::KptLinear<\d>, true>, cgp::KptUpdate<',
                    r'cgp::filter_kernel<cgp::EkfPredict<cgp::KptLinear<\d>, false>, cgp::KptUpdate<'),
    'kf4_mfma': r'cgp::kf4_mfma_kernel\(',
    'ekf4_mfma': r'cgp::ekf4_mfma_kernel\(',
    'ekf4_mfma_seg': r'cgp::ekf4_mfma_kernel\(',
    'ekf4_mfma_x4': r'cgp::ekf4_mfma_x4_kernel<',
    'ekf4_coop': r'cgp::ekf4_coop_kernel\(',
    'sgp4_mfma': r'cgp::sgp4_mfma_kernel<',
    'sgp4_coop': r'cgp::sgp4_coop_kernel<',
    'lane4_ekf': r'cgp::lane4_filter_kernel<cgp::EkfPredict<',
    'lane4_sgp': r'cgp::lane4_filter_kernel<cgp::SgpPredictLane<',
    'ekf8_coop': r'cgp::ekf8_coop_kernel<',
    'sgp8_coop': r'cgp::sgp8_coop_kernel<',
    'cdekf4_mfma': r'cgp::cdekf4_mfma_kernel\(',
    'cdekf4_coop': r'cgp::cdekf4_coop_kernel\(',
    'cdsgp4_mfma': r'cgp::cdsgp4_mfma_kernel<',
    'cdsgp4_coop': r'cgp::cdsgp4_coop_kernel<',
    'kpt8_coop': r'cgp::(kpt4_mfma|kpt8_coop)_kernel<',
    'coop8_linear': r'cgp::coop8_(smoother|split)_kernel<cgp::\w+Element<cgp::LinearDisc<',
    'coop8_harm': r'cgp::coop8_(smoother|split)_kernel<cgp::\w+Element<cgp::HarmonicLCD<',
    'walk4_linear': r'cgp::walk4_smoother_kernel<cgp::\w+Element<cgp::LinearDisc<4>',
    'walk4_harm': r'cgp::walk4_smoother_kernel<cgp::\w+Element<cgp::HarmonicLCD<1>',
    'lane4': r'cgp::lane4_smoother_kernel<',
    # (the generic smoothers with one wavefront per trial: the time-parallel scan, or step by step)
    'disc_linear': (r'cgp::(tp_smoother_kernel<cgp::\w+Element<cgp::LinearDisc<\d+>|smoother_kernel<cgp::\w+Step<cgp::LinearDisc<\d+>, true)',
                    r'cgp::smoother_kernel<cgp::\w+Step<cgp::LinearDisc<\d+>, false'),
    'disc_harm': (r'cgp::(tp_smoother_kernel<cgp::\w+Element<cgp::HarmonicLCD<\d+>|smoother_kernel<cgp::\w+Step<cgp::HarmonicLCD<\d+>, true)',
                  r'cgp::smoother_kernel<cgp::\w+Step<cgp::HarmonicLCD<\d+>, false'),
    'sde_linear': (r'cgp::smoother_kernel<cgp::Cd\w+Step<cgp::LinearSDE<\d+>, true', r'cgp::smoother_kernel<cgp::Cd\w+Step<cgp::LinearSDE<\d+>, false'),
    'sde_harm': (r'cgp::smoother_kernel<cgp::Cd\w+Step<cgp::HarmonicSDE<\d+>, true', r'cgp::smoother_kernel<cgp::Cd\w+Step<cgp::HarmonicSDE<\d+>, false'),
    'cdsgps4_mfma': r'cgp::cdsgps4_mfma_kernel<',
    'cdsgps4_coop': r'cgp::cdsgps4_coop_kernel<',
    'cdeks4_mfma': r'cgp::cdeks4_mfma_kernel<',
    'cdeks4_coop': r'cgp::cdeks4_coop_kernel\(',
}
# launches beside the routed kernel: the fix-up passes of the time-split entries
AUXILIARY = r'cgp::(filter_split_fixup_kernel|smoother_split_fixup_kernel)\('
# a smoother's line behind its route and shape: the plan (tests/route_probe.hip)
PLAN = r' tiles=(?P<tiles>\d+) bsegs=(?P<bsegs>\d+) chunks=\d+ burn=\d+ sel=(?P<sel>none|kernel|gather)'


def kernel_pattern(route_line):
    """'<route> wave=<w> segs=<n>[ <a smoother's plan>]' -> the compiled pattern of the kernel that route launches."""
    name, wave = re.fullmatch(r'(\w+) wave=([01]) segs=\d+(?:%s)?' % PLAN, route_line).group(1, 2)
    pattern = KERNELS[name]
    return re.compile(pattern if isinstance(pattern, str) else pattern[wave == '0'])


def kernels_fit(route_line, kernels):
    """The traced launches of a case are the route's kernel and fix-up passes.  A filter's kernel runs once or twice; a smoother's as its
    plan says: twice -- the compose and apply passes of the exact split -- where segs > 1, else once, and with the fix-up pass of the
    split with burn-in exactly where bsegs > 1."""
    pat = kernel_pattern(route_line)
    main = [k for k in kernels if not re.search(AUXILIARY, k)]
    plan = re.search(r' segs=(?P<segs>\d+)' + PLAN + '$', route_line)
    if plan:
        fixups = [k for k in kernels if 'smoother_split_fixup_kernel' in k]
        counts_fit = len(main) == (2 if int(plan['segs']) > 1 else 1) and len(fixups) == (1 if int(plan['bsegs']) > 1 else 0)
    else:
        counts_fit = 1 <= len(main) <= 2
    return counts_fit and all(pat.search(k) for k in main)


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)['cases']


@pytest.fixture(scope='module')
def probed(tmp_path_factory):
    """id -> the probe's line, for every case."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path_factory.mktemp('route_probe') / 'route_probe')
    subprocess.run([hipcc, '--cuda-host-only', '-O1', '-std=c++17', '-Wno-int-to-pointer-cast', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'route_probe.hip'), '-o', exe], check=True)
    lines = ''.join(rc.probe_line(c) + '\n' for c in rc.CASES)
    out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rc.CASES), (len(out), len(rc.CASES))
    return {c['id']: line for c, line in zip(rc.CASES, out)}


def test_golden_covers_the_case_list(golden):
    assert sorted(golden) == sorted(c['id'] for c in rc.CASES)
    for c in rc.CASES:
        g = golden[c['id']]
        assert bool(g.get('derived', False)) != c['run'], c['id']            # replayed on the GPU, or derived: never both
        assert c['run'] == ('kernels' in g), c['id']


def test_routes_are_the_recorded_ones(golden, probed):
    wrong = []
    for c in rc.CASES:
        want, got = golden[c['id']]['route'], probed[c['id']]
        if got != want:
            wrong.append(f"{c['id']}: {got!r}, recorded {want!r}")
    assert not wrong, f'{len(wrong)} of {len(rc.CASES)} routes differ:\n' + '\n'.join(wrong[:40])


def test_recorded_kernels_are_the_routes(golden):
    """The route names mean the kernels of the trace: every replayed case launched what its route says, a refused one nothing."""
    wrong = []
    for c in rc.CASES:
        g = golden[c['id']]
        if 'kernels' not in g:
            continue
        if g['route'].startswith('refused: '):
            ok = g['kernels'] == []
        else:
            ok = kernels_fit(g['route'], g['kernels'])
        if not ok:
            wrong.append(f"{c['id']}: {g['route']} against {g['kernels']}")
    assert not wrong, '\n'.join(wrong[:40])


def test_every_route_is_exercised(golden):
    seen = {g['route'].split()[0] for g in golden.values() if not g['route'].startswith('refused')}
    assert seen == set(KERNELS), (sorted(set(KERNELS) - seen), sorted(seen - set(KERNELS)))
    traced = {g['route'].split()[0] for g in golden.values() if g.get('kernels')}
    assert traced == set(KERNELS), sorted(set(KERNELS) - traced)


def test_crossovers_sit_where_they_were_measured(probed):
    """One trial below the quoted boundary runs one wavefront per trial, the boundary itself one lane per trial -- with 256 CUs and with 8."""
    for cid, _, _, _, _, _, num, den in rc.CROSSOVERS:
        for cus in (256, 8):
            first_lane = -(-num * 4 * cus // den)
            below, at = probed[f'x-{cid}-cu{cus}-B{first_lane - 1}'], probed[f'x-{cid}-cu{cus}-B{first_lane}']
            assert ' wave=1 ' in below and ' wave=0 ' in at, (cid, cus, below, at)
    for cus in (256, 8):                                                       # the literal 1024 of the four-trials-per-wavefront EKF
        assert probed[f'x-ekf4-x4-cu{cus}-B1024'].startswith('ekf4_mfma ') and probed[f'x-ekf4-x4-cu{cus}-B1025'].startswith('ekf4_mfma_x4 ')
