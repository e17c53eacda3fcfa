"""What the tests of the tangent entry points on records with gaps share (test_gaps_grad_fixture.py, test_gpu_gaps_gradient.py): the cases
of tests/golden/exact_gaps_grad.npz with their inputs from exact_grad_cases.npz, the engine call with missing='skip' along a case's
directions, and the C entry point itself with the caller's flags word and pre-filled output buffers (tests/tangent_cases.raw passes 0)."""
import ctypes as C
import os

import numpy as np

from tests.tangent_cases import GOLDEN, builder, directions, grad_case, run_dirs, sigma

ZGAPS = np.load(os.path.join(GOLDEN, 'exact_gaps_grad.npz'))
NAMES = [str(n) for n in ZGAPS['names']]
SKIP_MISSING = 0x2000      # include/chirpgp_hip.h: CGP_SKIP_MISSING


def gaps_case(name):
    """A case of exact_gaps_grad.npz: the source case's inputs (exact_grad_cases.npz), the record with its NaN, and the exact value, gradient
    and Fisher matrix of the observed samples; src_ys is the source's record."""
    src = str(ZGAPS[f'{name}.source'])
    c = grad_case(src)
    c['src_ys'] = c['ys']
    c.update({k: ZGAPS[f'{name}.{k}'] for k in ('ys', 'gaps', 'grad', 'fisher')})
    c.update({k: float(ZGAPS[f'{name}.{k}']) for k in ('nll', 'moved_nll', 'moved_grad', 'moved_fisher')})
    c.update({k: int(ZGAPS[f'{name}.{k}']) for k in ('n_dir', 'n_observed')})
    c.update(name=name, source=src, pattern=str(ZGAPS[f'{name}.pattern']), with_dxi=int(c['with_dxi']))
    return c


def case_dirs(c):
    """(1, n_dir, 24): the tangent directions at the case's theta and, where the case has d / d Xi, the direction whose only entry is dXi = 1."""
    D = directions(c)
    if c['with_dxi']:
        d7 = np.zeros((1, 1, 24))
        d7[0, 0, 9] = 1.0
        D = np.concatenate([D, d7], axis=1)
    return D


def run(c, fisher, ys=None, missing='skip', B=None):
    """E.run_{ekf,sgp}_nll_{grad,fisher} on records `ys` (T,) or (B, T) (default: the case's) at the case's theta, H and directions for every
    trial -> NumPy (nll (B,), grad (B, n_dir)[, fisher (B, n_dir, n_dir)])."""
    ys = c['ys'] if ys is None else np.asarray(ys, dtype=np.float64)
    B = (1 if ys.ndim == 1 else ys.shape[0]) if B is None else B
    thetas = np.tile(c['theta'], (B, 1))
    return run_dirs(c, np.tile(case_dirs(c), (B, 1, 1)), fisher=fisher, H=c['H'], thetas=thetas, ys=ys, missing=missing)


def raw(entry, c, ys, flags, fill=123.0, T=None):
    """The C entry point itself, one of tangent_cases.ENTRIES, with `flags`: records ys (B, T) (T = 0: pass T=0, ys is not read), the
    case's theta, H and directions for every trial, all three output buffers pre-filled with `fill`.
    -> (return code, message, nll (B,), grad (B, n_dir), fisher (B, n_dir, n_dir))."""
    import torch
    from chirpgp_amd import _engine as E, models as pm
    lib, ctx = E.load_library(), E.context()
    ys = np.atleast_2d(np.asarray(ys, dtype=np.float64))
    B = ys.shape[0]
    T = ys.shape[1] if T is None else T
    keep = []
    with np.errstate(all='ignore'):
        drift, disp, disc, m0, P0, H = builder(c['build'])(pm.g(c['theta']))
    dirs = case_dirs(c)[0]
    n_dir = int(dirs.shape[0])
    ys_d = E.dev(np.ascontiguousarray(ys))
    dirs_d = E.dev(np.ascontiguousarray(np.tile(dirs.reshape(-1), B)))
    opts = dict(dtype=torch.float64, device='cuda')
    nll, grad, F = torch.full((B,), fill, **opts), torch.full((B, n_dir), fill, **opts), torch.full((B, n_dir, n_dir), fill, **opts)
    model, init = E._model_struct(disc, None, B, keep), E._init_struct(c['H'], c['Xi'], m0, P0, 4, B, keep)
    args = [ctx, C.byref(model)]
    if '_sgp_' in entry:
        args.append(C.byref(E._sigma_struct(sigma(c['sigma'] or 'cubature'), 4, keep, None)))
    args += [C.byref(init), c['dt'], ys_d.data_ptr(), int(ys.shape[1]), 1, None, B, T, dirs_d.data_ptr(), n_dir, nll.data_ptr(), grad.data_ptr()]
    args += ([F.data_ptr()] if entry.endswith('_fisher') else []) + [flags, E._stream()]
    rc = getattr(lib, entry)(*args)
    torch.cuda.synchronize()
    msg = lib.cgp_last_error(ctx) if rc else b''
    return rc, msg, nll.cpu().numpy(), grad.cpu().numpy(), F.cpu().numpy()
