"""The case table of tests/abi_cases.py through the real library, with real small device buffers: every row that is not `derived` returns
the code and the message of tests/golden/abi_refusals.json and leaves every pre-filled output bit for bit as it was -- a refused or an
empty call enqueues nothing -- and each entry point's one good call returns 0 and writes its outputs.

One row supersedes the golden file: 'cgp_filter_time_split: segments = 1, ys = NULL'.  The library that recorded the file zeroed
junction_err before it had checked anything, and the file says so ('writes'); since the checks come first, a refused call writes nothing,
and that is what is asserted here."""
import os

import numpy as np
import pytest

from tests import abi_cases as ac
from tests.test_abi_refusals import golden_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# outputs that are added into (atomics): an element whose sum is zero keeps its pre-fill, as 74 of the 208 Cramer-Rao sums of this call do
ACCUMULATED = {'sums4', 'sums26'}


@pytest.fixture(scope='module')
def device():
    from chirpgp_amd import _engine as E
    dev = ac.Device(E.load_library(), E.context(), os.path.join(ROOT, 'chirpgp_amd', 'csrc'))
    yield dev
    dev.close()


@pytest.mark.parametrize('entry', list(ac.ENTRIES))
def test_refusals_and_empty_calls(device, entry):
    golden = golden_rows()
    superseded = [cid for cid, g in golden.items() if g.get('writes')]
    assert superseded == ['cgp_filter_time_split: segments = 1, ys = NULL']
    ran = 0
    for cid, edit, derived in ac.rows(entry):
        if derived:
            continue
        rc, msg, outs = device.run(entry, edit)
        print(f'{cid}: {rc} {msg}')
        assert (rc, msg) == (golden[cid]['rc'], golden[cid]['message']), cid
        for name, after in outs.items():
            assert device.untouched(name, after), (cid, name)
        ran += 1
    assert ran > 0


@pytest.mark.parametrize('entry', list(ac.ENTRIES))
def test_good_calls_write_every_output(device, entry):
    rc, msg, outs = device.run(entry)
    assert rc == 0, msg
    for name, after in outs.items():
        left = int((after == device.host[name]).sum())
        print(f'{entry}: {name} keeps {left} of {after.size} pre-filled elements')
        if name in ACCUMULATED:
            assert left < after.size and np.isfinite(after).all(), (entry, name)
        else:
            assert left == 0, (entry, name, left)
