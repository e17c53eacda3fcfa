"""The argument checks the four tangent entry points share (csrc/cgp_args.hpp: prepare_tangent): one faulty argument at a time gives the same
return code from every entry point that takes the argument, and leaves the output buffers as they were.  Beside them two good calls:
T = 9 crosses the EKF kernel's 8-step measurement block, T = 0 writes zeros.

The rows are those of the C-ABI's case table (tests/abi_cases.py: TANGENT_FAULTS), whose codes are those the four hand-written copies of
the checks returned before they were folded (recorded on an MI355X with that commit's library: every row, for all four entry points)."""
import numpy as np
import numpy.testing as npt
import pytest

from tests.abi_cases import E_UNSUPPORTED, TANGENT_FAULTS as FAULTS
from tests.tangent_cases import ENTRIES, ZG, directions, grad_case, raw

pytestmark = pytest.mark.gpu
VALUE_RTOL, GRAD_GATE = 1e-11, 1e-8                # the gates of test_gpu_gradient_edges.py::test_record_lengths, which runs T = 9 through mle
FILL = 123.0


@pytest.mark.parametrize('entry', ENTRIES)
def test_shared_argument_checks(entry):
    """B = 1, T = 8, n_dir = 6, the chirp model and the cubature set, output buffers pre-filled."""
    sgp, fisher = '_sgp_' in entry, entry.endswith('_fisher')
    name = 'prefix_cubature' if sgp else 'prefix_ekf'
    c = grad_case(name)
    assert c['build'] == 'chirp' and c['sigma'] == ('cubature' if sgp else '')
    dirs = directions(c)[0]
    assert dirs.shape == (6, 24)
    for label, edit, code, sigma_only in FAULTS:
        if sigma_only and not sgp:
            continue
        rc, msg, nll, grad, F = raw(entry, c, 8, dirs, FILL, edit=edit)
        print(f'{entry}, {label}: {rc} {msg.decode() if msg else ""}')
        assert rc == code, (label, rc, msg)
        assert code != E_UNSUPPORTED or entry.encode() in msg, (label, msg)                 # a refusal names its own entry point
        for out in (nll, grad, F):
            npt.assert_array_equal(out, FILL, err_msg=label)
    # ---- the good calls
    rc, msg, nll, grad, F = raw(entry, c, 9, dirs, FILL)
    assert rc == 0, msg
    want_f, want_g = ZG[f'{name}.nll_prefix'][8], ZG[f'{name}.grad_prefix'][8]
    ev, eg = abs(nll[0] - want_f) / abs(want_f), np.abs(grad[0] - want_g).max() / np.abs(want_g).max()
    print(f'{entry}, T = 9: value error {ev:.2e}, gradient error {eg:.2e} of its scale')
    assert ev < VALUE_RTOL and eg < GRAD_GATE, (nll, want_f, grad, want_g)
    if fisher:
        assert np.isfinite(F).all() and (np.diag(F[0]) > 0).all()
        npt.assert_array_equal(F, F.transpose(0, 2, 1))
    else:
        npt.assert_array_equal(F, FILL)
    rc, msg, nll, grad, F = raw(entry, c, 0, dirs, FILL)
    assert rc == 0, msg
    npt.assert_array_equal(nll, 0.0)
    npt.assert_array_equal(grad, 0.0)
    npt.assert_array_equal(F, 0.0 if fisher else FILL)
