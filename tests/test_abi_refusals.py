"""What every C-ABI entry point makes of a faulty or an empty call is pinned, without a GPU: the pure half of the entry points
(csrc/cgp_args.hpp: the prepare_ functions), asked through the host program tests/abi_probe.hip, answers every row of tests/abi_cases.py
as tests/golden/abi_refusals.json records it -- the return code and the message, byte for byte -- and lets every good call through.

The golden file: what the library of the commit BEFORE the entry points were split into a pure prepare step and their launch returned, row
by row, driven through ctypes with real small device buffers on an MI355X; the rows marked "derived" (limits that no device buffer can
reach, a model of a second device, a kind of run-time model the device test does not compile) have their code and message read off that
commit's source, and say so.  The probe links no HIP runtime: cgp_args.hpp calls none."""
import json
import os
import shutil
import subprocess

import pytest

from tests import abi_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'abi_refusals.json')


def golden_rows():
    with open(GOLDEN) as fh:
        return json.load(fh)['rows']


def expected_line(g):
    """A golden row as the probe prints it."""
    return f"refused {g['rc']}: {g['message']}" if g['rc'] else 'empty'


@pytest.fixture(scope='module')
def golden():
    return golden_rows()


@pytest.fixture(scope='module')
def probed(tmp_path_factory):
    """(entry, row id or None for the good call) -> the probe's line."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path_factory.mktemp('abi_probe') / 'abi_probe')
    subprocess.run([hipcc, '--cuda-host-only', '-no-hip-rt', '-O1', '-std=c++17', '-Wno-int-to-pointer-cast', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'abi_probe.hip'), '-o', exe], check=True)
    keys, lines = [], []
    for entry in ac.ENTRIES:
        keys.append((entry, None))
        lines.append(ac.probe_line(entry, ac.arguments(entry)))
        for cid, edit, _ in ac.rows(entry):
            keys.append((entry, cid))
            lines.append(ac.probe_line(entry, ac.arguments(entry, edit)))
    out = subprocess.run([exe], input=''.join(line + '\n' for line in lines), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(keys), (len(out), len(keys))
    return dict(zip(keys, out))


def test_golden_covers_the_case_table(golden):
    ids = [cid for entry in ac.ENTRIES for cid, _, _ in ac.rows(entry)]
    assert len(set(ids)) == len(ids)
    assert sorted(golden) == sorted(ids)
    for entry in ac.ENTRIES:
        for cid, _, derived in ac.rows(entry):
            g = golden[cid]
            assert bool(g.get('derived', False)) == derived, cid               # recorded on the GPU, or read off the source: never both
            assert (g['rc'] == 0) == (g['message'] == ''), cid
            assert g['rc'] in (0, ac.E_ARG, ac.E_UNSUPPORTED), cid           # nothing in the table reaches a launch


def test_every_entry_point_has_its_rows():
    """Every exported entry point that launches is in the table, with an empty call wherever it has one."""
    from chirpgp_amd import _engine as E
    host_only = {'cgp_version', 'cgp_create', 'cgp_destroy', 'cgp_last_error', 'cgp_source_hash', 'cgp_debug_set', 'cgp_debug_counters',
                 'cgp_reserve_workspace', 'cgp_release_workspace', 'cgp_model_from_source', 'cgp_custom_model_destroy'}
    assert set(ac.ENTRIES) == set(E.EXPORTS) - host_only
    for entry, spec in ac.ENTRIES.items():
        labels = [r[0] for r in spec['rows']]
        tangent = 'n_dir' in spec['good']                # its empty calls are B = 0 and n_dir = 0: T = 0 launches, and writes zeros
        for size in ('B', 'T', 'n', 'n_dir'):
            if size in spec['good'] and not (size == 'n' and 'B' in spec['good']) and not (size == 'T' and tangent):
                assert f'{size} = 0' in labels, (entry, size)


def test_refusals_are_the_recorded_ones(golden, probed):
    wrong = []
    for entry in ac.ENTRIES:
        for cid, _, _ in ac.rows(entry):
            want, got = expected_line(golden[cid]), probed[(entry, cid)]
            if got != want:
                wrong.append(f'{cid}: {got!r}, recorded {want!r}')
    assert not wrong, f'{len(wrong)} rows differ:\n' + '\n'.join(wrong[:40])


def test_good_calls_reach_the_launch(probed):
    for entry in ac.ENTRIES:
        assert probed[(entry, None)] == 'ok', (entry, probed[(entry, None)])


def test_the_tangent_rows_keep_their_codes(golden):
    """The rows tests/test_gpu_tangent_arguments.py shares carry the codes that test asserts on the device."""
    for entry in ('cgp_ekf_nll_grad', 'cgp_sgp_nll_grad', 'cgp_ekf_nll_fisher', 'cgp_sgp_nll_fisher', 'cgp_cd_ekf_nll_grad'):
        for label, _, code, sigma_only in ac.TANGENT_FAULTS:
            if sigma_only and '_sgp_' not in entry:
                continue
            assert golden[f'{entry}: {label}']['rc'] == code, (entry, label)
