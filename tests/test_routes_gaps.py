"""Which kernel a cgp_filter call with CGP_SKIP_MISSING takes: only one that honours the flag (csrc/cgp_route.hpp: honours_gaps) -- the
generic kernel in the shape the call has, or the one-wavefront-per-trial matrix-core kernels of ekf / sgp_filter / cd_ekf / cd_sgp_filter
at d = 4 -- and a time-split call is refused.  Asked through the host probe of tests/test_routes.py (tests/route_probe.hip); no GPU."""
import os
import shutil
import subprocess

import pytest

from tests import route_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP = 0x2000                                            # CGP_SKIP_MISSING (include/chirpgp_hip.h)


def q(method, model, sigma=None, B=4, T=128, flags=0, entry='filter', segments=1, align=0):
    # (a dict of our own: route_cases.case() would append to the pinned list)
    return dict(entry=entry, method=method, model=model, sigma=sigma, B=B, T=T, flags=flags | SKIP, segments=segments, align=align, num_cus=256,
                null_rows=False)


QUERIES = {
    # the d = 4 chirp family: the matrix-core kernels, whose launchers take the kernel for records with gaps
    'ekf-chirp': (q('ekf', 'chirp'), 'ekf4_mfma wave=1 segs=1'),
    'ekf-lascala': (q('ekf', 'lascala'), 'ekf4_mfma wave=1 segs=1'),
    'sgp-chirp': (q('sgp', 'chirp', 'gh3'), 'sgp4_mfma wave=1 segs=1'),
    'cd_ekf-chirp': (q('cd_ekf', 'chirp_sde1'), 'cdekf4_mfma wave=1 segs=1'),
    'cd_sgp-chirp': (q('cd_sgp', 'chirp_sde1', 'gh3'), 'cdsgp4_mfma wave=1 segs=1'),
    # never the four-trials-per-wavefront EKF
    'ekf-chirp-b1025-wave': (q('ekf', 'chirp', B=1025, T=64, flags=rc.WAVE), 'ekf4_mfma wave=1 segs=1'),
    'ekf-chirp-b1025': (q('ekf', 'chirp', B=1025, T=64), 'ekf4_mfma wave=1 segs=1'),
    'ekf-chirp-four': (q('ekf', 'chirp', flags=rc.FOUR_TRIALS), 'ekf4_mfma wave=1 segs=1'),
    # what falls back: the tile layout (d = 6 / 8, KPT), kf at d = 4, the DPP variants, the sets the matrix-core quadrature does not take
    'sgp-harm3': (q('sgp', 'harm3', 'cub'), 'generic_wave wave=1 segs=1'),
    'ekf-harm2': (q('ekf', 'harm2'), 'generic_wave wave=1 segs=1'),
    'kf-linear4': (q('ekf', 'linear4'), 'generic_wave wave=1 segs=1'),
    'kpt2': (q('ekf_kpt', 'kpt2'), 'generic_kpt wave=1 segs=1'),
    'kpt3-thread': (q('ekf_kpt', 'kpt3', B=70, flags=rc.THREAD), 'generic_kpt wave=0 segs=1'),
    'ekf-chirp-dpp': (q('ekf', 'chirp', flags=rc.DPP), 'generic_wave wave=1 segs=1'),
    'ekf-chirp-generic': (q('ekf', 'chirp', flags=rc.GENERIC), 'generic_wave wave=1 segs=1'),
    'sgp-chirp-dpp': (q('sgp', 'chirp', 'gh3', flags=rc.DPP), 'generic_wave wave=1 segs=1'),
    'cd_ekf-chirp-dpp': (q('cd_ekf', 'chirp_sde1', flags=rc.DPP), 'generic_wave wave=1 segs=1'),
    'sgp-chirp-ungrouped': (q('sgp', 'chirp', 'ungrouped'), 'generic_wave wave=1 segs=1'),
    'sgp-chirp-generic': (q('sgp', 'chirp', 'gh3', flags=rc.GENERIC), 'generic_wave wave=1 segs=1'),
    # one lane per trial: the generic kernel, never the large-batch lane kernels
    'ekf-chirp-thread': (q('ekf', 'chirp', B=70, flags=rc.THREAD), 'generic_lane wave=0 segs=1'),
    'sgp-chirp-thread': (q('sgp', 'chirp', 'gh3', B=70, flags=rc.THREAD), 'generic_lane wave=0 segs=1'),
    # the crossovers of flagged calls on 256 CUs: measured for ekf (5.5 trials per SIMD) and sgp_filter (21) on the chirp model, the
    # generic ones ({5, 2}; sigma-point {8, 1}) for everything else
    'ekf-chirp-b5631': (q('ekf', 'chirp', B=5631, T=64), 'ekf4_mfma wave=1 segs=1'),
    'ekf-chirp-b5632': (q('ekf', 'chirp', B=5632, T=64), 'generic_lane wave=0 segs=1'),
    'sgp-chirp-b21503': (q('sgp', 'chirp', 'gh3', B=21503, T=64), 'sgp4_mfma wave=1 segs=1'),
    'sgp-chirp-b21504': (q('sgp', 'chirp', 'gh3', B=21504, T=64), 'generic_lane wave=0 segs=1'),
    'cd_ekf-chirp-b2559': (q('cd_ekf', 'chirp_sde1', B=2559, T=64), 'cdekf4_mfma wave=1 segs=1'),
    'cd_ekf-chirp-b2560': (q('cd_ekf', 'chirp_sde1', B=2560, T=64), 'generic_lane wave=0 segs=1'),
    'cd_sgp-chirp-b8191': (q('cd_sgp', 'chirp_sde1', 'gh3', B=8191, T=64), 'cdsgp4_mfma wave=1 segs=1'),
    'cd_sgp-chirp-b8192': (q('cd_sgp', 'chirp_sde1', 'gh3', B=8192, T=64), 'generic_lane wave=0 segs=1'),
    'ekf-harm2-b2560': (q('ekf', 'harm2', B=2560, T=64), 'generic_lane wave=0 segs=1'),
    # time-split with burn-in: refused, whatever the kernel could do without the flag
    'fsplit-ekf': (q('ekf', 'chirp', T=256, entry='filter_split', segments=2), 'refused'),
    'fsplit-sgp': (q('sgp', 'chirp', 'gh3', T=256, entry='filter_split', segments=2), 'refused'),
}


@pytest.fixture(scope='module')
def probed(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path_factory.mktemp('route_probe_gaps') / 'route_probe')
    subprocess.run([hipcc, '--cuda-host-only', '-O1', '-std=c++17', '-Wno-int-to-pointer-cast', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'route_probe.hip'), '-o', exe], check=True)
    ids = list(QUERIES)
    lines = ''.join(rc.probe_line(QUERIES[i][0]) + '\n' for i in ids)
    out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ids), out
    return dict(zip(ids, out))


@pytest.mark.parametrize('cid', list(QUERIES))
def test_flagged_route(probed, cid):
    want, got = QUERIES[cid][1], probed[cid]
    if want == 'refused':
        assert got.startswith('refused: ') and 'CGP_SKIP_MISSING' in got, got          # the message names the flag
    else:
        assert got == want, (cid, got, want)


def test_the_pinned_case_list_is_untouched():
    assert not any(c['flags'] & SKIP for c in rc.CASES)
