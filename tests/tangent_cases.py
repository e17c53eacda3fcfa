"""What the tests of the four tangent entry points -- cgp_ekf_nll_grad, cgp_sgp_nll_grad, cgp_ekf_nll_fisher, cgp_sgp_nll_fisher -- share
(test_gpu_gradient_edges.py, test_gpu_fisher.py): the cases of the two 100-digit fixtures, the builders and sigma-point sets they name,
the engine call with the caller's directions and the C entry point itself with pre-filled output buffers."""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ZG = np.load(os.path.join(GOLDEN, 'exact_grad_cases.npz'))
ZF = np.load(os.path.join(GOLDEN, 'exact_fisher.npz'))
ENTRIES = ('cgp_ekf_nll_grad', 'cgp_sgp_nll_grad', 'cgp_ekf_nll_fisher', 'cgp_sgp_nll_fisher')


def grad_case(name):
    """A case of exact_grad_cases.npz."""
    keys = ('theta', 'ys', 'Xi', 'dt', 'H', 'build', 'method', 'sigma', 'nll', 'grad', 'group', 'lost', 'with_dxi', 'moved_nll', 'moved_grad')
    c = {k: ZG[f'{name}.{k}'] for k in keys}
    for k in ('Xi', 'dt', 'nll', 'moved_nll', 'moved_grad'):
        c[k] = float(c[k])
    for k in ('build', 'method', 'sigma', 'group'):
        c[k] = str(c[k])
    c['name'] = name
    return c


def fisher_case(name):
    """A case of exact_fisher.npz: its inputs from exact_grad_cases.npz (the first T samples of the source's record), the exact F, and the
    exact value and gradient at that record length."""
    src, T = str(ZF[f'{name}.source']), int(ZF[f'{name}.T'])
    c = {k: ZG[f'{src}.{k}'] for k in ('theta', 'ys', 'H', 'with_dxi')}
    c.update({k: float(ZG[f'{src}.{k}']) for k in ('Xi', 'dt')})
    c.update({k: str(ZG[f'{src}.{k}']) for k in ('build', 'method', 'sigma')})
    if T == c['ys'].size:
        c['nll'], c['grad'] = float(ZG[f'{src}.nll']), ZG[f'{src}.grad']
    else:
        c['nll'], c['grad'] = float(ZG[f'{src}.nll_prefix'][T - 1]), ZG[f'{src}.grad_prefix'][T - 1]
    c.update(name=name, ys=c['ys'][:T], fisher=ZF[f'{name}.fisher'], with_dxi=int(c['with_dxi']))
    return c


def builder(name):
    from chirpgp_amd import models as pm
    return pm.build_chirp_model if name == 'chirp' else pm.build_lascala_model


def sigma(name):
    from chirpgp_amd.quadratures import SigmaPoints
    if not name:
        return None
    return SigmaPoints.cubature(4) if name == 'cubature' else SigmaPoints.gauss_hermite(4, int(name[2:]))


def directions(c, thetas=None):
    from chirpgp_amd import mle
    return mle.tangent_directions(builder(c['build']), c['theta'][None, :] if thetas is None else thetas, c['dt'], c['Xi'])


def run_dirs(c, dirs, fisher=False, T=None, H=None, Xi=None, m0=None, P0=None, thetas=None, ys=None, **kw):
    """The raw engine call E.run_*_nll_grad (fisher: E.run_*_nll_fisher) with the caller's directions (B, n_dir, 24) and, on request, its
    own H / Xi / m0 / P0, parameter vectors and records (default: the case's first T measurements)."""
    from chirpgp_amd import _engine as E, models as pm
    thetas = c['theta'][None, :] if thetas is None else thetas
    with np.errstate(all='ignore'):
        drift, disp, disc, m0_, P0_, H_ = builder(c['build'])(pm.g(thetas))
    H, Xi, m0, P0 = (H_ if H is None else H), (c['Xi'] if Xi is None else Xi), (m0_ if m0 is None else m0), (P0_ if P0 is None else P0)
    ys = (c['ys'] if T is None else c['ys'][:T]) if ys is None else ys
    tail = 'fisher' if fisher else 'grad'
    if c['method'] == 'ekf':
        out = getattr(E, f'run_ekf_nll_{tail}')(disc, H, Xi, m0, P0, c['dt'], ys, dirs, **kw)
    else:
        out = getattr(E, f'run_sgp_nll_{tail}')(disc, sigma(c['sigma']), H, Xi, m0, P0, c['dt'], ys, dirs, **kw)
    return tuple(o.cpu().numpy() for o in out)


def raw(entry, c, T, dirs, fill=123.0, B=1, sg=None, P0=None, edit=None):
    """The C entry point itself, one of ENTRIES, on the case's first T measurements with `dirs` (n_dir, 24) for every trial and all three
    output buffers pre-filled with `fill` (the gradient entry points are not handed the third).  `edit(a)` may change the arguments
    before the call: a dict of the structs `model`, `sigma`, `init` and of `ys`, `ys_stride`, `ys_repeat`, `ys_index`, `B`, `T`, `dirs`,
    `n_dir`, `nll`, `grad`, `fisher` (pointers as integers; None is NULL).
    -> (return code, message, nll (B,), grad (B, n_dir), fisher (B, n_dir, n_dir)), the buffers sized for one trial where B = 0."""
    import torch
    from chirpgp_amd import _engine as E, models as pm
    lib, ctx = E.load_library(), E.context()
    keep, rows = [], max(B, 1)
    drift, disp, disc, m0, P0_, H = builder(c['build'])(pm.g(c['theta']))
    ys = E.dev(np.ascontiguousarray(c['ys'][:max(T, 1)]))
    n_dir = int(dirs.shape[0])
    dirs_d = E.dev(np.ascontiguousarray(np.tile(dirs.reshape(-1), rows)))
    opts = dict(dtype=torch.float64, device='cuda')
    nll, grad, F = torch.full((rows,), fill, **opts), torch.full((rows, n_dir), fill, **opts), torch.full((rows, n_dir, n_dir), fill, **opts)
    a = dict(model=E._model_struct(disc, None, rows, keep), init=E._init_struct(H, c['Xi'], m0, P0_ if P0 is None else P0, 4, rows, keep),
             sigma=E._sigma_struct(sg if sg is not None else sigma(c['sigma'] or 'cubature'), 4, keep, None) if '_sgp_' in entry else None,
             ys=ys.data_ptr(), ys_stride=max(T, 1), ys_repeat=1, ys_index=None, B=B, T=T, dirs=dirs_d.data_ptr(), n_dir=n_dir,
             nll=nll.data_ptr(), grad=grad.data_ptr(), fisher=F.data_ptr())
    if edit is not None:
        edit(a)
    ref = lambda s: None if s is None else C.byref(s)
    args = [ctx, ref(a['model'])] + ([ref(a['sigma'])] if '_sgp_' in entry else []) + [ref(a['init']), c['dt']]
    args += [a[k] for k in ('ys', 'ys_stride', 'ys_repeat', 'ys_index', 'B', 'T', 'dirs', 'n_dir', 'nll', 'grad')]
    args += ([a['fisher']] if entry.endswith('_fisher') else []) + [0, E._stream()]
    rc = getattr(lib, entry)(*args)
    torch.cuda.synchronize()
    msg = lib.cgp_last_error(ctx) if rc else b''
    return rc, msg, nll.cpu().numpy(), grad.cpu().numpy(), F.cpu().numpy()
