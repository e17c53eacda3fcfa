"""A test of the test: the arena of tests/guard_bands.py on CPU tensors -- what it reports, where it puts a payload, how large its guards
are -- and, as tests/test_routes_gaps.py does for the flagged calls, the coverage of the GPU sweep (tests/test_gpu_guard_bands.py: SWEEP)
pinned through the host probe tests/route_probe.hip: every case reaches the route it states, in both placements, and the routes the sweep
reaches are all there are (tests/test_routes.py: KERNELS).  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import guard_bands as gb
from tests import route_cases as rc
from tests import test_gpu_guard_bands as sweep
from tests import test_routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def as_words(t):
    return t.view(-1).view(torch.int64)


# ---- the arena --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('placement', gb.PLACEMENTS)
def test_a_clean_launch_reports_nothing(placement):
    arena = gb.Arena('cpu', placement)
    src = np.arange(12.).reshape(3, 4)
    x = arena.input(src, 'ys')
    out = arena.output((3, 4), 'mfs')
    assert x.is_contiguous() and out.is_contiguous() and x.dtype == out.dtype == torch.float64
    assert np.array_equal(x.numpy(), src)
    assert bool((as_words(out) == gb.PREFILL).all())
    out.copy_(2 * x)
    assert arena.check() == []
    assert arena.requests == [('mfs', (3, 4))]


@pytest.mark.parametrize('placement', gb.PLACEMENTS)
def test_planted_violations_are_reported_with_name_and_position(placement):
    arena = gb.Arena('cpu', placement)
    out = arena.output((5, 7), 'Pfs')
    ys = arena.input(np.ones(9), 'ys')
    out.fill_(1.)
    assert arena.check() == []
    block = arena.blocks[0]
    # one word in the front guard, three words before the payload; one in the back guard of the INPUT, right behind it
    block.words[block.offset - 3] = 0
    ys_block = arena.blocks[1]
    ys_block.words[ys_block.offset + ys_block.n] = 0
    # one output word left unwritten
    as_words(out)[2 * 7 + 4] = gb.PREFILL
    found = arena.check()
    assert len(found) == 3, found
    front, back, unwritten = found
    assert front.startswith('Pfs (5, 7) front guard: 1 words changed, 24 .. 24 bytes before the payload'), front
    assert back.startswith('ys (9,) back guard: 1 words changed, 8 .. 8 bytes behind the payload'), back
    assert unwritten == 'Pfs (5, 7): 1 of 35 words never written, first at [(2, 4)]', unwritten
    assert arena.written() == [('Pfs', 34)]
    # the far ends of the guards count too
    block.words[0] = 1
    block.words[-1] = 1
    found = arena.guard_violations()
    assert f'{block.offset * 8} bytes before' in found[0] and f'{(block.words.numel() - block.offset - block.n) * 8} bytes behind' in found[1], found


def test_a_nan_the_kernel_computed_is_not_an_unwritten_word():
    arena = gb.Arena('cpu', 'aligned')
    out = arena.output((4,), 'nll')
    out.copy_(torch.tensor([1., float('nan'), -float('nan'), float('inf')], dtype=torch.float64))
    words = as_words(out)
    words[1] = gb.CANONICAL_NAN
    assert bool(torch.isnan(out[1])) and arena.check() == []
    # ... and both patterns are quiet NaNs of their own
    for pattern in (gb.GUARD, gb.PREFILL):
        assert pattern != gb.CANONICAL_NAN and pattern >> 51 == 0xFFF and np.isnan(np.array([pattern], dtype=np.int64).view(np.float64)[0])
    assert gb.GUARD != gb.PREFILL


def test_an_untouched_output_is_all_unwritten_and_written_is_empty():
    arena = gb.Arena('cpu', 'odd')
    arena.output((2, 3), 'grad')
    assert arena.written() == [] and arena.guard_violations() == []
    assert arena.check() == ['grad (2, 3): 6 of 6 words never written, first at [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]']


@pytest.mark.parametrize('shape', [(1,), (3, 5), (129, 48, 4, 4), (8192,), (8193,)])
def test_placements_and_guard_sizes(shape):
    n = int(np.prod(shape))
    for placement, fits in (('aligned', lambda p: p % 256 == 0), ('odd', lambda p: p % 16 == 8)):
        arena = gb.Arena('cpu', placement)
        for t in (arena.output(shape, 'o'), arena.input(np.zeros(shape), 'i'), arena.input(np.zeros(shape), 'k', placement='aligned')):
            assert tuple(t.shape) == shape
        o, i, k = arena.blocks
        assert fits(o.payload.data_ptr()) and fits(i.payload.data_ptr()) and k.payload.data_ptr() % 256 == 0, placement
        for b in arena.blocks:
            for _, words in b.guards:
                assert words.numel() * 8 >= max(64 * 1024, n * 8), (shape, placement)
            assert b.payload.data_ptr() == b.words.data_ptr() + 8 * b.offset
    assert gb.guard_words(1) == 8192 and gb.guard_words(8193) == 8193


def test_the_context_manager_installs_and_restores_the_seam():
    from chirpgp_amd import _engine
    before = _engine._new_output
    arena = gb.Arena('cpu', 'odd')
    with pytest.raises(KeyError):
        with arena.installed():
            t = _engine._new_output((2, 3), torch.device('cpu'), 'mss')
            assert t.data_ptr() % 16 == 8 and arena.requests == [('mss', (2, 3))]
            raise KeyError
    assert _engine._new_output is before
    plain = _engine._new_output((2, 3), 'cpu')
    assert plain.dtype == torch.float64 and tuple(plain.shape) == (2, 3) and plain.device.type == 'cpu'


def test_same_bits_tells_nan_payloads_apart():
    a = torch.tensor([1., float('nan')], dtype=torch.float64)
    b = a.clone()
    assert gb.same_bits(a, b) and gb.same_bits(None, None) and not gb.same_bits(a, None)
    b.view(torch.int64)[1] = gb.GUARD
    assert not gb.same_bits(a, b)


# ---- the sweep's coverage ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def probed():
    """(case id, placement) -> the probe's line."""
    import tempfile
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    keys = [(c, p) for c in sweep.SWEEP for p in gb.PLACEMENTS]
    models = rc.MODELS
    rc.MODELS = sweep.MODELS                                   # (probe_line looks the model up there: two more linear ones)
    try:
        lines = ''.join(rc.probe_line(sweep.probe_query(c, p)) + '\n' for c, p in keys)
    finally:
        rc.MODELS = models
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, 'route_probe')
        subprocess.run([hipcc, '--cuda-host-only', '-O1', '-std=c++17', '-Wno-int-to-pointer-cast', '-I', os.path.join(ROOT, 'include'),
                        os.path.join(ROOT, 'tests', 'route_probe.hip'), '-o', exe], check=True)
        out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(keys), (len(out), len(keys))
    return {(c['id'], p): line for (c, p), line in zip(keys, out)}


def test_every_case_reaches_the_route_it_states(probed):
    wrong = []
    for c in sweep.SWEEP:
        for p in gb.PLACEMENTS:
            line = probed[c['id'], p]
            if not line.startswith(f"{c['route']} wave={c['wave']} "):
                wrong.append(f"{c['id']} ({p}): {line!r}, meant {c['route']} wave={c['wave']}")
                continue
            plan = re.search(r' segs=(\d+)(?: tiles=\d+ bsegs=(\d+))?', line)
            pieces = max(int(plan.group(1)), int(plan.group(2) or 1))
            if c['entry'] == 'filter_split' and pieces < 2:
                wrong.append(f"{c['id']} ({p}): {line!r} is not split")
            if c['split'] is not None and (pieces > 1) != c['split']:
                wrong.append(f"{c['id']} ({p}): {line!r}, split meant to be {c['split']}")
            if c['entry'] == 'select' and not line.endswith('sel=gather' if c['route'].startswith('disc') else 'sel=kernel'):
                wrong.append(f"{c['id']} ({p}): {line!r}: the selection is written the other way")
    assert not wrong, f'{len(wrong)} cases:\n' + '\n'.join(wrong[:40])


def test_the_sweep_reaches_every_route():
    assert {c['route'] for c in sweep.SWEEP} == set(test_routes.KERNELS)


def test_the_sweep_covers_what_it_promises():
    """The shapes and subsets the sweep is there for, counted where they are easy to lose."""
    by_route = {}
    for c in sweep.SWEEP:
        by_route.setdefault(c['route'], []).append(c)
    assert len(sweep.FULL) == 11 and len(sweep.ALL7) == 7 and len(sweep.SELECTIONS) == 7
    for route in ('ekf4_mfma', 'ekf4_mfma_seg', 'ekf4_mfma_x4', 'ekf4_coop', 'kf4_mfma', 'sgp4_mfma', 'sgp4_coop', 'cdekf4_mfma', 'cdekf4_coop',
                  'cdsgp4_mfma', 'cdsgp4_coop', 'lane4_ekf', 'lane4_sgp'):
        assert any(c['run'].get('variants') is sweep.FULL for c in by_route[route]), route
    for route in ('lane4_ekf', 'lane4_sgp'):
        assert {(c['B'], c['T']) for c in by_route[route]} >= set(sweep.LANE_SHAPES)
        assert any(c['run'].get('ridx') for c in by_route[route]) and any(c['run'].get('records') == 1 for c in by_route[route])
    assert {(c['B'], c['T']) for c in by_route['lane4'] if c['entry'] == 'smoother'} >= set(sweep.LANE_SHAPES)
    assert any(c['run'].get('missing') == 'skip' and c['T'] == 65 for c in by_route['ekf4_mfma'])
    for wave in (0, 1):
        assert any(c['wave'] == wave for c in by_route['generic_kpt']) and any(c['wave'] == wave for c in by_route['disc_linear'])
    assert {c['entry'] for c in sweep.SWEEP} == {'filter', 'filter_split', 'smoother', 'smoother_split', 'select'}
    # the lane kernels are the only ones whose admission looks at an input's alignment: nothing else needs its inputs kept aligned
    assert {c['route'] for c in sweep.SWEEP if c['keep_aligned']} == {'lane4_ekf', 'lane4_sgp', 'lane4'}


def test_the_pinned_case_list_is_untouched():
    assert 'linear5' not in rc.MODELS and not any(c['flags'] & sweep.SKIP for c in rc.CASES)
