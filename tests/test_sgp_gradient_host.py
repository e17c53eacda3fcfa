"""The sigma-point filter's exact-gradient entry point (cgp_sgp_nll_grad) on the host side: declared, exported, refuses a NULL context
without a GPU, and mle.has_exact_gradient admits exactly the combinations the kernel is built for."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'chirpgp_hip.h')


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from chirpgp_amd import _engine
    return _engine.load_library(), _engine


def test_declared_in_the_header_and_exported():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert re.search(r'\bint\s+cgp_sgp_nll_grad\s*\(', src)
    lib, eng = _lib()
    assert 'cgp_sgp_nll_grad' in eng.EXPORTS
    assert hasattr(lib, 'cgp_sgp_nll_grad')


def test_null_context_is_an_argument_error_without_a_gpu():
    lib, _ = _lib()
    assert lib.cgp_sgp_nll_grad(None, None, None, None, 1e-3, None, 0, 1, None, 1, 10, None, 6, None, None, 0, None) == -1


def test_has_exact_gradient_for_the_sigma_point_filter():
    from chirpgp_amd import mle, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    gh3, cub = SigmaPoints.gauss_hermite(4, 3), SigmaPoints.cubature(4)
    for sg in (gh3, cub):
        assert mle.has_exact_gradient('sgp_filter', pm.build_chirp_model, 0.1, sgps=sg)
        assert mle.has_exact_gradient('sgp_filter', pm.build_lascala_model, 0.1, sgps=sg)
    assert not mle.has_exact_gradient('sgp_filter', pm.build_chirp_model, 0.1)
    assert not mle.has_exact_gradient('sgp_filter', pm.build_chirp_model, 0.1, sgps=SigmaPoints.cubature(6))
    assert not mle.has_exact_gradient('sgp_filter', pm.build_harmonic_chirp_model, 0.1, sgps=gh3)
    assert not mle.has_exact_gradient('sgp_filter', pm.build_chirp_model, np.array([0.1, 0.2]), sgps=gh3)
    assert not mle.has_exact_gradient('cd_sgp_filter', pm.build_chirp_model, 0.1, sgps=gh3)
    assert mle.has_exact_gradient('ekf', pm.build_chirp_model, 0.1)          # the EKF's route is unchanged
    # exact=None keeps the difference form for the sigma-point filter whatever the batch
    assert not mle._exact_by_default('sgp_filter', pm.build_chirp_model, 0.1, 10 ** 6, {})
