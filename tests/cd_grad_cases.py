"""What the tests of cgp_cd_ekf_nll_grad share (test_cd_gradient_host.py, test_gpu_cd_gradient.py): the cases of the 100-digit fixture
tests/golden/exact_cd_grad.npz, the gates, and the C entry point itself with pre-filled output buffers (tests/tangent_cases.py: raw, for
the continuous-discrete form)."""
import ctypes as C
import os

import numpy as np

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'exact_cd_grad.npz'))
NAMES = [str(n) for n in Z['names']]
ENTRY = 'cgp_cd_ekf_nll_grad'
VALUE_RTOL, GRAD_GATE = 1e-11, 1e-8                    # the project's gates for the discrete tangent kernels (tests/test_gpu_gradient_edges.py:35)
VALUE_MOVE_MAX, GRAD_MOVE_MAX = 1e-13, 1e-10           # the generator's admission limits
PREFIX_T = (1, 2, 7, 8, 9, 64, 65, 130)                # across the eight-step measurement block
SKIP_MISSING = 0x2000                                  # include/chirpgp_hip.h: CGP_SKIP_MISSING


def case(name):
    keys = ('theta', 'ys', 'Xi', 'dt', 'H', 'build', 'method', 'nll', 'grad', 'group', 'lost', 'with_dxi', 'skip', 'moved_nll', 'moved_grad')
    c = {k: Z[f'{name}.{k}'] for k in keys}
    for k in ('Xi', 'dt', 'nll', 'moved_nll', 'moved_grad'):
        c[k] = float(c[k])
    for k in ('build', 'method', 'group'):
        c[k] = str(c[k])
    for k in ('lost', 'with_dxi', 'skip'):
        c[k] = int(c[k])
    c['name'] = name
    return c


def gates(c):
    """(value gate, gradient gate): the fixed ones; for a case exempt from admission max(gate, 100 x its stored movement)."""
    if c['group'] == 'edge':
        return max(VALUE_RTOL, 100.0 * c['moved_nll']), max(GRAD_GATE, 100.0 * c['moved_grad'])
    return VALUE_RTOL, GRAD_GATE


def errors(f, grad, want_f, want_g, label):
    """(value relative error, gradient error over its largest component), printed; a reference that is exactly zero (a record of NaN
    only) is compared absolutely."""
    scale = np.abs(want_g).max()
    ev = abs(f - want_f) / (abs(want_f) if want_f != 0 else 1.0)
    eg = float(np.abs(grad - want_g).max() / (scale if scale != 0 else 1.0))
    print(f'{label}: value error {ev:.2e}, gradient error {eg:.2e} of its scale {scale:.3g}')
    return ev, eg


def builder(name):
    from chirpgp_amd import models as pm
    return pm.build_chirp_model if name == 'chirp' else pm.build_lascala_model


def directions(c, thetas=None):
    """mle.tangent_directions_cd at the case's theta -- with the direction whose only entry is d Xi = 1 as a seventh where the case has it."""
    from chirpgp_amd import mle
    d = mle.tangent_directions_cd(builder(c['build']), c['theta'][None, :] if thetas is None else thetas, c['dt'], c['Xi'])
    if c['with_dxi'] and thetas is None:
        d7 = np.zeros((1, 1, 27))
        d7[0, 0, 12] = 1.0
        d = np.concatenate([d, d7], axis=1)
    return d


def raw(c, T, dirs, fill=123.0, B=1, flags=0, P0=None, edit=None):
    """The C entry point itself on the case's first T measurements with `dirs` (n_dir, 27) for every trial and both output buffers
    pre-filled with `fill`.  `edit(a)` may change the arguments before the call: a dict of the structs `model`, `init` and of `ys`,
    `ys_stride`, `ys_repeat`, `ys_index`, `B`, `T`, `dirs`, `n_dir`, `nll`, `grad`, `flags` (pointers as integers; None is NULL).
    -> (return code, message, nll (B,), grad (B, n_dir)), the buffers sized for one trial where B = 0."""
    import torch
    from chirpgp_amd import _engine as E, models as pm
    lib, ctx = E.load_library(), E.context()
    keep, rows = [], max(B, 1)
    # (a batch of one, as mle builds it: NumPy's array and scalar powers differ in the last bit of the dispersion's 2 sigma gam^1.5)
    drift, disp, disc, m0, P0_, H = builder(c['build'])(pm.g(c['theta'][None, :]))
    P0 = None if P0 is None else np.asarray(P0)[None]
    ys = E.dev(np.ascontiguousarray(c['ys'][:max(T, 1)]))
    n_dir = int(dirs.shape[0])
    dirs_d = E.dev(np.ascontiguousarray(np.tile(dirs.reshape(-1), rows)))
    opts = dict(dtype=torch.float64, device='cuda')
    nll, grad = torch.full((rows,), fill, **opts), torch.full((rows, n_dir), fill, **opts)
    a = dict(model=E._model_struct(drift, disp.outer(), rows, keep), init=E._init_struct(c['H'], c['Xi'], m0, P0_ if P0 is None else P0, 4, rows, keep),
             ys=ys.data_ptr(), ys_stride=max(T, 1), ys_repeat=1, ys_index=None, B=B, T=T, dirs=dirs_d.data_ptr(), n_dir=n_dir,
             nll=nll.data_ptr(), grad=grad.data_ptr(), flags=flags)
    if edit is not None:
        edit(a)
    ref = lambda s: None if s is None else C.byref(s)
    args = [ctx, ref(a['model']), ref(a['init']), c['dt']] + [a[k] for k in ('ys', 'ys_stride', 'ys_repeat', 'ys_index', 'B', 'T', 'dirs', 'n_dir', 'nll', 'grad', 'flags')]
    rc = getattr(lib, ENTRY)(*args, E._stream())
    torch.cuda.synchronize()
    msg = lib.cgp_last_error(ctx) if rc else b''
    return rc, msg, nll.cpu().numpy(), grad.cpu().numpy()
