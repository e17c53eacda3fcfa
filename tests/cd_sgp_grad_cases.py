"""What the tests of cgp_sgp_nll_grad on the SDE model share (test_cd_sgp_gradient_host.py, test_gpu_cd_sgp_gradient.py): the cases of the
100-digit fixture tests/golden/exact_cd_sgp_grad.npz, the gates, the sigma-point sets by name, and the C entry point itself with
pre-filled output buffers (tests/cd_grad_cases.py: raw, with the sigma-point set)."""
import ctypes as C
import os

import numpy as np

from tests.cd_grad_cases import GRAD_GATE, GRAD_MOVE_MAX, SKIP_MISSING, VALUE_MOVE_MAX, VALUE_RTOL, builder, errors      # noqa: F401 (shared)

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'exact_cd_sgp_grad.npz'))
NAMES = [str(n) for n in Z['names']]
ENTRY = 'cgp_sgp_nll_grad'
PREFIX_T = (1, 2, 63, 64, 65, 128, 129, 130)           # across the 64-step measurement chunk of the wave-per-trial kernel
PREFIX_NAMES = ('prefix_cds_cubature', 'prefix_cds_gh3')


def rk4_substeps(n):
    """include/chirpgp_hip.h: CGP_RK4_SUBSTEPS(n)."""
    from chirpgp_amd import _engine as E
    return E.rk4_substeps(n)


def case(name):
    keys = ('theta', 'ys', 'Xi', 'dt', 'H', 'build', 'method', 'sigma', 'nll', 'grad', 'group', 'lost', 'with_dxi', 'skip', 'n', 'moved_nll', 'moved_grad')
    c = {k: Z[f'{name}.{k}'] for k in keys}
    for k in ('Xi', 'dt', 'nll', 'moved_nll', 'moved_grad'):
        c[k] = float(c[k])
    for k in ('build', 'method', 'group', 'sigma'):
        c[k] = str(c[k])
    for k in ('lost', 'with_dxi', 'skip', 'n'):
        c[k] = int(c[k])
    c['name'] = name
    return c


def gates(c):
    """(value gate, gradient gate): the fixed ones; for a case exempt from admission max(gate, 100 x its stored movement)."""
    if c['group'] == 'edge':
        return max(VALUE_RTOL, 100.0 * c['moved_nll']), max(GRAD_GATE, 100.0 * c['moved_grad'])
    return VALUE_RTOL, GRAD_GATE


def sigma_points(name):
    """'cubature' (8 points), 'gh3' (81), 'gh4' (256), 'gh5' (625): the library's d = 4 sets."""
    from chirpgp_amd.quadratures import SigmaPoints
    return SigmaPoints.cubature(4) if name == 'cubature' else SigmaPoints.gauss_hermite(4, int(name[2:]))


def directions(c, thetas=None):
    """mle.tangent_directions_cd at the case's theta -- with the direction whose only entry is d Xi = 1 as a seventh where the case has it."""
    from chirpgp_amd import mle
    d = mle.tangent_directions_cd(builder(c['build']), c['theta'][None, :] if thetas is None else thetas, c['dt'], c['Xi'])
    if c['with_dxi'] and thetas is None:
        d7 = np.zeros((1, 1, 27))
        d7[0, 0, 12] = 1.0
        d = np.concatenate([d, d7], axis=1)
    return d


def raw(c, T, dirs, fill=123.0, B=1, flags=0, P0=None, edit=None, entry=ENTRY):
    """The C entry point itself on the case's first T measurements with `dirs` (n_dir, 27) for every trial, the case's sigma-point set and
    both output buffers pre-filled with `fill`.  `edit(a)` may change the arguments before the call: a dict of the structs `model`,
    `sigma`, `init` and of `ys`, `ys_stride`, `ys_repeat`, `ys_index`, `B`, `T`, `dirs`, `n_dir`, `nll`, `grad`, `flags` (pointers as
    integers; None is NULL).  entry = 'cgp_sgp_nll_fisher': with a third buffer.  -> (return code, message, nll (B,), grad (B, n_dir))."""
    import torch
    from chirpgp_amd import _engine as E, models as pm
    lib, ctx = E.load_library(), E.context()
    keep, rows = [], max(B, 1)
    drift, disp, disc, m0, P0_, H = builder(c['build'])(pm.g(np.repeat(c['theta'][None, :], rows, axis=0)))      # (a batch, as mle builds it)
    P0 = None if P0 is None else np.asarray(P0)
    ys = E.dev(np.ascontiguousarray(c['ys'][:max(T, 1)]))
    n_dir = int(dirs.shape[0])
    dirs_d = E.dev(np.ascontiguousarray(np.tile(dirs.reshape(-1), rows)))
    opts = dict(dtype=torch.float64, device='cuda')
    nll, grad, fisher = torch.full((rows,), fill, **opts), torch.full((rows, n_dir), fill, **opts), torch.full((rows, n_dir, n_dir), fill, **opts)
    a = dict(model=E._model_struct(drift, disp.outer(), rows, keep), sigma=E._sigma_struct(sigma_points(c['sigma']), 4, keep, None),
             init=E._init_struct(c['H'], c['Xi'], m0, P0_ if P0 is None else P0, 4, rows, keep),
             ys=ys.data_ptr(), ys_stride=max(T, 1), ys_repeat=rows, ys_index=None, B=B, T=T, dirs=dirs_d.data_ptr(), n_dir=n_dir,
             nll=nll.data_ptr(), grad=grad.data_ptr(), flags=flags)
    if edit is not None:
        edit(a)
    ref = lambda s: None if s is None else C.byref(s)
    outs = [a['nll'], a['grad']] + ([fisher.data_ptr()] if entry.endswith('fisher') else [])
    args = [ctx, ref(a['model']), ref(a['sigma']), ref(a['init']), c['dt']] + [a[k] for k in ('ys', 'ys_stride', 'ys_repeat', 'ys_index', 'B', 'T', 'dirs', 'n_dir')]
    rc = getattr(lib, entry)(*args, *outs, a['flags'], E._stream())
    torch.cuda.synchronize()
    msg = lib.cgp_last_error(ctx) if rc else b''
    return rc, msg, nll.cpu().numpy(), grad.cpu().numpy()
