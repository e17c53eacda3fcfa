"""ctypes binding of libchirpgp_hip.so (include/chirpgp_hip.h) and the marshalling shared by the public functions.

PyTorch-ROCm is used for device memory, streams and torch.distributed only: every array handed to the library is a
``torch.Tensor.data_ptr()`` of a float64 CUDA(HIP) tensor; no torch op takes part in the arithmetic.  There is no
CPU path: a missing library or GPU raises.
"""
import ctypes as C
import os
import threading
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libchirpgp_hip.so')

# enumerations of include/chirpgp_hip.h
F_EKF, F_SGP, F_CD_EKF, F_CD_SGP, F_EKF_KPT = range(5)
S_EKS, S_SGP, S_CD_EKS, S_CD_SGP = range(4)
M_LINEAR, M_HARMONIC_LCD, M_LASCALA_LCD, M_LINEAR_SDE, M_HARMONIC_SDE, M_KPT = range(6)
NLL_FINAL_ONLY, WAVE_PER_TRIAL, THREAD_PER_TRIAL, SEQUENTIAL_SCAN, GENERIC_KERNEL, SIM_FIXED_X0 = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
LITERAL_SIGMA_SUM, DPP_KERNEL, FOUR_TRIALS_PER_WAVE, ONE_TRIAL_PER_WAVE = 0x40, 0x80, 0x200, 0x400
TIME_SPLIT, NO_TIME_SPLIT, SKIP_MISSING = 0x800, 0x1000, 0x2000
RK4_SUBSTEPS_MASK, MAX_SUBSTEPS = 0x000F0000, 16      # CGP_RK4_SUBSTEPS(n) = (n - 1) << 16, n = 1 .. 16
SIGMA_STANDARD = 0x1
SIGMA_AXIAL = 0x2
MAX_D = 12            # include/chirpgp_hip.h: CGP_MAX_D (9 .. 12: the harmonic LCD model with 4 or 5 harmonics)


def _check_dimension(spec):
    d = int(spec.d)
    limit = MAX_D if int(spec.model_id) == M_HARMONIC_LCD else 8
    if d > limit:
        raise NotImplementedError(f'state dimension {d} > {limit} is not compiled into libchirpgp_hip.so for this model')
    return d

_vp = C.c_void_p


class CgpModel(C.Structure):
    _fields_ = [('model_id', C.c_int32), ('d', C.c_int32), ('n_harm', C.c_int32), ('n_params', C.c_int32),
                ('params', _vp), ('param_stride', C.c_int64), ('gamma', _vp), ('gamma_stride', C.c_int64)]


class CgpSigma(C.Structure):
    _fields_ = [('s', C.c_int32), ('d', C.c_int32), ('xi', _vp), ('w', _vp), ('group_start', _vp), ('n_groups', C.c_int32),
                ('flags', C.c_uint32)]


class CgpInit(C.Structure):
    _fields_ = [('H', _vp), ('H_stride', C.c_int64), ('Xi', _vp), ('Xi_stride', C.c_int64),
                ('m0', _vp), ('m0_stride', C.c_int64), ('P0', _vp), ('P0_stride', C.c_int64)]


class CgpSmoothOut(C.Structure):
    _fields_ = [('mss', _vp), ('Pss', _vp), ('comp', C.c_int32), ('func', C.c_int32), ('comp_mean', _vp), ('comp_var', _vp),
                ('expect', _vp), ('xi', _vp), ('w', _vp), ('order', C.c_int32)]


class CgpSampleOut(C.Structure):
    _fields_ = [('paths', _vp), ('comp_paths', _vp), ('comp', C.c_int32), ('func', C.c_int32)]


EXPORTS = ('cgp_version', 'cgp_create', 'cgp_destroy', 'cgp_last_error', 'cgp_filter', 'cgp_smoother',
           'cgp_gaussian_expectation', 'cgp_debug_math', 'cgp_simulate', 'cgp_add_noise', 'cgp_debug_philox',
           'cgp_debug_set', 'cgp_debug_counters', 'cgp_gaussian_expectation_fn', 'cgp_filter_time_split', 'cgp_squared_error_sums',
           'cgp_reserve_workspace', 'cgp_release_workspace', 'cgp_source_hash', 'cgp_smoother_select', 'cgp_ekf_nll_grad', 'cgp_sgp_nll_grad', 'cgp_ekf_nll_fisher', 'cgp_sgp_nll_fisher', 'cgp_cd_ekf_nll_grad', 'cgp_model_from_source', 'cgp_custom_model_destroy',
           'cgp_filter_custom', 'cgp_smoother_custom', 'cgp_smoother_time_split', 'cgp_smoother_sample', 'cgp_pcrlb_sums', 'cgp_simulate_x0')

# include/chirpgp_hip_timed.h: the continuous-discrete methods with one interval per step.  A tuple of its own: EXPORTS is chirpgp_hip.h's.
TIMED_EXPORTS = ('cgp_filter_timed', 'cgp_smoother_timed')
TIMED_VERSION = 1      # CGP_TIMED_VERSION

_lib = None
_lock = threading.Lock()


def load_library():
    """dlopen libchirpgp_hip.so and declare the prototypes.  Raises if the library has not been built."""
    global _lib
    # torch first: PyTorch-ROCm ships its own libamdhip64; loading it before our library makes both use the same HIP
    # runtime (the reverse order leaves two runtimes in the process and hipGetDeviceCount fails in ours).
    _torch()
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                               f'or `make -C chirpgp_amd/csrc` (there is no CPU fallback)')
        lib = C.CDLL(LIB_PATH)
        lib.cgp_version.restype = C.c_int
        lib.cgp_create.restype = C.c_int
        lib.cgp_create.argtypes = [C.POINTER(_vp), C.c_int]
        lib.cgp_destroy.restype = None
        lib.cgp_destroy.argtypes = [_vp]
        lib.cgp_last_error.restype = C.c_char_p
        lib.cgp_last_error.argtypes = [_vp]
        lib.cgp_filter.restype = C.c_int
        lib.cgp_filter.argtypes = [_vp, C.c_int, C.POINTER(CgpModel), C.POINTER(CgpSigma), C.POINTER(CgpInit), C.c_double,
                                   _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_uint32, _vp]
        lib.cgp_filter_time_split.restype = C.c_int
        lib.cgp_filter_time_split.argtypes = [_vp, C.c_int, C.POINTER(CgpModel), C.POINTER(CgpSigma), C.POINTER(CgpInit), C.c_double,
                                              _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_uint32,
                                              C.c_int64, C.c_int64, _vp, _vp]
        lib.cgp_smoother.restype = C.c_int
        lib.cgp_smoother.argtypes = [_vp, C.c_int, C.POINTER(CgpModel), C.POINTER(CgpSigma), C.c_double,
                                     _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, C.c_uint32, _vp]
        lib.cgp_smoother_time_split.restype = C.c_int
        lib.cgp_smoother_time_split.argtypes = [_vp, C.c_int, C.POINTER(CgpModel), C.POINTER(CgpSigma), C.c_double, _vp, _vp, C.c_int64, C.c_int64,
                                                _vp, _vp, C.c_uint32, C.c_int64, C.c_int64, _vp, _vp]
        lib.cgp_smoother_select.restype = C.c_int
        lib.cgp_smoother_select.argtypes = [_vp, C.c_int, C.POINTER(CgpModel), C.POINTER(CgpSigma), C.c_double,
                                            _vp, _vp, C.c_int64, C.c_int64, C.POINTER(CgpSmoothOut), C.c_uint32, _vp]
        lib.cgp_filter_timed.restype = C.c_int
        lib.cgp_filter_timed.argtypes = [_vp, C.c_int, C.POINTER(CgpModel), C.POINTER(CgpSigma), C.POINTER(CgpInit), _vp, C.c_int64,
                                         _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_uint32, _vp]
        lib.cgp_smoother_timed.restype = C.c_int
        lib.cgp_smoother_timed.argtypes = [_vp, C.c_int, C.POINTER(CgpModel), C.POINTER(CgpSigma), _vp, C.c_int64, C.c_int64, _vp,
                                           _vp, _vp, C.c_int64, C.c_int64, C.POINTER(CgpSmoothOut), C.c_uint32, _vp]
        lib.cgp_smoother_sample.restype = C.c_int
        lib.cgp_smoother_sample.argtypes = [_vp, C.c_int, C.POINTER(CgpModel), C.POINTER(CgpSigma), C.c_double, _vp, _vp, C.c_int64, C.c_int64, C.c_int64,
                                            C.c_uint64, C.c_int64, C.c_int64, _vp, C.POINTER(CgpSampleOut), C.c_uint32, _vp]
        lib.cgp_ekf_nll_grad.restype = C.c_int
        lib.cgp_ekf_nll_grad.argtypes = [_vp, C.POINTER(CgpModel), C.POINTER(CgpInit), C.c_double, _vp, C.c_int64, C.c_int64, _vp,
                                         C.c_int64, C.c_int64, _vp, C.c_int32, _vp, _vp, C.c_uint32, _vp]
        lib.cgp_sgp_nll_grad.restype = C.c_int
        lib.cgp_sgp_nll_grad.argtypes = [_vp, C.POINTER(CgpModel), C.POINTER(CgpSigma), C.POINTER(CgpInit), C.c_double, _vp, C.c_int64, C.c_int64,
                                         _vp, C.c_int64, C.c_int64, _vp, C.c_int32, _vp, _vp, C.c_uint32, _vp]
        lib.cgp_ekf_nll_fisher.restype = C.c_int
        lib.cgp_ekf_nll_fisher.argtypes = [_vp, C.POINTER(CgpModel), C.POINTER(CgpInit), C.c_double, _vp, C.c_int64, C.c_int64, _vp,
                                           C.c_int64, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp, C.c_uint32, _vp]
        lib.cgp_sgp_nll_fisher.restype = C.c_int
        lib.cgp_sgp_nll_fisher.argtypes = [_vp, C.POINTER(CgpModel), C.POINTER(CgpSigma), C.POINTER(CgpInit), C.c_double, _vp, C.c_int64, C.c_int64,
                                           _vp, C.c_int64, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp, C.c_uint32, _vp]
        lib.cgp_cd_ekf_nll_grad.restype = C.c_int
        lib.cgp_cd_ekf_nll_grad.argtypes = lib.cgp_ekf_nll_grad.argtypes
        lib.cgp_model_from_source.restype = C.c_int
        lib.cgp_model_from_source.argtypes = [_vp, C.c_int, C.c_int32, C.c_char_p, C.c_char_p, C.POINTER(_vp)]
        lib.cgp_custom_model_destroy.restype = None
        lib.cgp_custom_model_destroy.argtypes = [_vp]
        lib.cgp_filter_custom.restype = C.c_int
        lib.cgp_filter_custom.argtypes = [_vp, _vp, C.POINTER(CgpSigma), _vp, C.c_int64, _vp, C.c_int64, C.POINTER(CgpInit), C.c_double, _vp, C.c_int64, C.c_int64, _vp,
                                          C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_uint32, _vp]
        lib.cgp_smoother_custom.restype = C.c_int
        lib.cgp_smoother_custom.argtypes = [_vp, _vp, C.POINTER(CgpSigma), _vp, C.c_int64, _vp, C.c_int64, C.c_double, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, C.c_uint32, _vp]
        lib.cgp_gaussian_expectation.restype = C.c_int
        lib.cgp_gaussian_expectation.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, C.c_int32, _vp, _vp]
        lib.cgp_gaussian_expectation_fn.restype = C.c_int
        lib.cgp_gaussian_expectation_fn.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, C.c_int32, _vp, _vp]
        lib.cgp_squared_error_sums.restype = C.c_int
        lib.cgp_squared_error_sums.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_int32, _vp, _vp]
        lib.cgp_pcrlb_sums.restype = C.c_int
        lib.cgp_pcrlb_sums.argtypes = [_vp, C.POINTER(CgpModel), C.c_double, _vp, _vp, C.c_int64, C.c_int64, _vp, C.c_uint32, _vp]
        lib.cgp_simulate_x0.restype = C.c_int
        lib.cgp_simulate_x0.argtypes = [_vp, C.POINTER(CgpModel), C.POINTER(CgpInit), C.c_uint64, C.c_int64, C.c_int64, _vp, _vp]
        lib.cgp_debug_math.restype = C.c_int
        lib.cgp_debug_math.argtypes = [_vp, C.c_int, _vp, C.c_int64, _vp, _vp, _vp]
        lib.cgp_simulate.restype = C.c_int
        lib.cgp_simulate.argtypes = [_vp, C.POINTER(CgpModel), C.POINTER(CgpInit), C.c_double, C.c_uint64, C.c_int64,
                                     C.c_int64, C.c_int64, _vp, _vp, C.c_uint32, _vp]
        lib.cgp_add_noise.restype = C.c_int
        lib.cgp_add_noise.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, _vp, _vp]
        lib.cgp_debug_philox.restype = C.c_int
        lib.cgp_debug_set.restype = C.c_int
        lib.cgp_debug_set.argtypes = [_vp, C.c_int, C.c_int64]
        lib.cgp_debug_counters.restype = C.c_int
        lib.cgp_debug_counters.argtypes = [_vp, C.POINTER(C.c_uint64), C.c_int, _vp]
        lib.cgp_debug_philox.argtypes = [_vp, _vp, _vp, C.c_int64, _vp, _vp]
        lib.cgp_reserve_workspace.restype = C.c_int
        lib.cgp_reserve_workspace.argtypes = [_vp, C.c_size_t, _vp]
        lib.cgp_release_workspace.restype = C.c_int
        lib.cgp_release_workspace.argtypes = [_vp, _vp]
        lib.cgp_source_hash.restype = C.c_char_p
        lib.cgp_source_hash.argtypes = []
        built_from, tree = lib.cgp_source_hash().decode(), source_hash()
        if tree is not None and built_from != tree:
            raise RuntimeError(f'{LIB_PATH} is stale: built from sources {built_from[:16]}..., the checked-out csrc/ + include/ hash to '
                               f'{tree[:16]}... -- rebuild it (`make -C chirpgp_amd/csrc`); there is no CPU fallback')
        _lib = lib
        return lib


def source_hash():
    """sha256 of the sources a library of this tree is built from -- csrc/*.hip, csrc/*.hpp (byte order of the names), csrc/Makefile,
    include/chirpgp_hip.h, include/chirpgp_hip_timed.h, concatenated: what csrc/Makefile embeds as cgp_source_hash().  None where the sources are not shipped
    (a binary-only install), in which case nothing can be compared."""
    import glob
    import hashlib
    src = os.path.join(_HERE, 'csrc')
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(src, '*.hip')) + glob.glob(os.path.join(src, '*.hpp')))
    include = os.path.join(os.path.dirname(_HERE), 'include')
    files = [os.path.join(src, n) for n in names] + [os.path.join(src, 'Makefile'), os.path.join(include, 'chirpgp_hip.h'),
                                                     os.path.join(include, 'chirpgp_hip_timed.h')]
    if not names or not all(os.path.exists(f) for f in files):
        return None
    h = hashlib.sha256()
    for f in files:
        with open(f, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


_contexts = {}


def _torch():
    import torch
    return torch


def context(device_index=None):
    """One cgp_ctx per (process, device)."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError('chirpgp_amd needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback')
    if device_index is None:
        device_index = torch.cuda.current_device()
    with _lock:
        ctx = _contexts.get(device_index)
    if ctx is None:
        lib = load_library()
        h = _vp()
        rc = lib.cgp_create(C.byref(h), int(device_index))
        if rc != 0:
            raise RuntimeError(f'cgp_create(device={device_index}) failed with {rc}')
        with _lock:
            ctx = _contexts.setdefault(device_index, h)
    return ctx


def _check(ctx, rc, what):
    if rc != 0:
        msg = load_library().cgp_last_error(ctx)
        raise RuntimeError(f'{what} failed ({rc}): {msg.decode() if msg else "?"}')


def _is_torch(x):
    return type(x).__module__.startswith('torch')


def dev(x, device=None):
    """-> contiguous float64 tensor on the GPU (uploading NumPy input)."""
    torch = _torch()
    if _is_torch(x):
        t = x
        if not t.is_cuda:
            t = t.cuda(device) if device is not None else t.cuda()
        return t.to(torch.float64).contiguous()
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    t = torch.from_numpy(a)
    return t.cuda(device) if device is not None else t.cuda()


_const_cache = {}


# Optional timing hook used by bench.py: when set to a list, every kernel launch appends
# (name, start_event, end_event), the events recorded on the launch stream immediately around the C-ABI call.
kernel_events = None


def _timed(name, call):
    if kernel_events is None:
        return call()
    torch = _torch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = call()
    e1.record()
    kernel_events.append((name, e0, e1))
    return rc


def dev_const(x):
    """Device copy of a small host constant (model parameters, H, m0, P0, sigma points), cached by value so that
    repeated calls with the same model do not pay a pageable host-to-device copy (which would also serialise the
    host behind the previous kernel)."""
    if _is_torch(x):
        return dev(x)
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if a.size > 8192:
        return dev(a)
    key = (_torch().cuda.current_device(), a.shape, a.tobytes())
    t = _const_cache.get(key)
    if t is None:
        if len(_const_cache) >= 512:
            _const_cache.clear()
        t = _const_cache[key] = dev(a)
    return t


def _index_const(a):
    """Device copy of a small int32 index array, cached by value like dev_const (a lock-step line search passes the same
    few index sets again and again; an uncached pageable upload would serialise the host behind the previous kernel)."""
    torch = _torch()
    if a.size > 65536:
        return torch.from_numpy(a).cuda()
    key = (torch.cuda.current_device(), 'i32', a.shape, a.tobytes())
    t = _const_cache.get(key)
    if t is None:
        if len(_const_cache) >= 512:
            _const_cache.clear()
        t = _const_cache[key] = torch.from_numpy(a).cuda()
    return t


def _ptr(t):
    return _vp(t.data_ptr()) if t is not None else None


def _stream():
    return _vp(_torch().cuda.current_stream().cuda_stream)


def _batched_operand(x, base_ndim, B, name):
    """Device tensor of an operand that is shared (base_ndim dims) or per-trial (leading B); returns (tensor, stride)."""
    t = dev_const(x)
    if t.ndim == base_ndim:
        return t, 0
    if t.ndim == base_ndim + 1 and t.shape[0] == B:
        per = 1
        for s in t.shape[1:]:
            per *= int(s)
        return t, per
    raise ValueError(f'{name}: expected {base_ndim} dims (shared) or a leading batch axis of {B}, got shape {tuple(t.shape)}')


def _model_operands(spec, gamma, B, keep):
    """The model's device operands: (params, param_stride, b b^T or None, its stride)."""
    params = dev_const(spec.params)
    if params.ndim == 2 and params.shape[0] != B:
        raise ValueError(f'model parameters have batch {params.shape[0]} but the data has batch {B}')
    keep.append(params)
    g, gs = None, 0
    if gamma is not None:
        g, gs = _batched_operand(gamma, 2, B, 'dispersion')
        if tuple(g.shape[-2:]) != (spec.d, spec.d):
            raise ValueError(f'b b^T must be {spec.d} x {spec.d}, got {tuple(g.shape)}')
        keep.append(g)
    return params, (int(params.shape[-1]) if params.ndim == 2 else 0), g, gs


def _model_struct(spec, gamma, B, keep):
    params, pstride, g, gs = _model_operands(spec, gamma, B, keep)
    m = CgpModel()
    m.model_id, m.d, m.n_harm, m.n_params = int(spec.model_id), int(spec.d), int(spec.n_harm), int(params.shape[-1])
    m.params, m.param_stride = _ptr(params), pstride
    if g is not None:
        m.gamma, m.gamma_stride = _ptr(g), gs
    return m


_sigma_cache = {}


def _sigma_struct(sgps, d, keep, nonlinear_coord=None):
    """cgp_sigma for a SigmaPoints.  With `nonlinear_coord` = v (the chirp models: v = d - 2) the points are reordered so
    that points sharing xi[0..v] are contiguous and the group boundaries are passed along: the kernels then evaluate the
    transcendental part of the model once per group (include/chirpgp_hip.h, cgp_sigma).  Reordering only changes the
    order of summation."""
    if sgps is None:
        return None
    torch = _torch()
    xi_h, w_h = np.asarray(sgps.xi, dtype=np.float64), np.asarray(sgps.w, dtype=np.float64)
    if xi_h.ndim != 2 or xi_h.shape[1] != d or w_h.shape != (xi_h.shape[0],):
        raise ValueError(f'sigma points must be (s, {d}) with (s,) weights; got {xi_h.shape}, {w_h.shape}')
    key = (torch.cuda.current_device(), nonlinear_coord, xi_h.shape, xi_h.tobytes(), w_h.tobytes())
    hit = _sigma_cache.get(key)
    if hit is None:
        gs, sflags = None, 0
        if nonlinear_coord is not None:
            v = int(nonlinear_coord)
            prefix = xi_h[:, :v + 1] + 0.0          # exact grouping (-0.0 folded into +0.0)
            _, inverse = np.unique(prefix, axis=0, return_inverse=True)
            order = np.argsort(inverse.ravel(), kind='stable')
            xi_h, w_h, inv = xi_h[order], w_h[order], inverse.ravel()[order]
            starts = np.flatnonzero(np.r_[True, inv[1:] != inv[:-1], True]).astype(np.int32)
            gs = torch.from_numpy(starts).cuda()
            sflags = SIGMA_STANDARD if _is_standard(xi_h, w_h, starts, v) else 0
            if sflags and (np.count_nonzero(xi_h[:, :d - 1], axis=1) <= 1).all():
                sflags |= SIGMA_AXIAL            # cubature: every point on one axis (include/chirpgp_hip.h)
        if len(_sigma_cache) >= 64:
            _sigma_cache.clear()
        hit = _sigma_cache[key] = (dev(xi_h), dev(w_h), gs, sflags)
    xi, w, gs, sflags = hit
    keep += [xi, w, gs]
    return CgpSigma(int(xi.shape[0]), int(d), _ptr(xi), _ptr(w), _ptr(gs), int(gs.numel() - 1) if gs is not None else 0, sflags)


def _is_standard(xi, w, starts, v, tol=1e-13):
    """The assertion behind CGP_SIGMA_STANDARD (include/chirpgp_hip.h): unit weight, zero mean, identity second moment,
    and groups whose members differ in the last coordinate only, with zero weighted mean there."""
    d = xi.shape[1]
    if v != d - 2:
        return False
    if abs(w.sum() - 1) > tol or np.abs(w @ xi).max() > tol or np.abs((xi.T * w) @ xi - np.eye(d)).max() > tol:
        return False
    for a, b in zip(starts[:-1], starts[1:]):
        if np.abs(xi[a:b, :d - 1] - xi[a, :d - 1]).max() != 0 or abs(w[a:b] @ xi[a:b, d - 1]) > tol * 0.1:
            return False
    return True


def _nonlinear_coord(spec):
    """State coordinate the model is nonlinear in (chirp / harmonic / La Scala models: d - 2), None for linear models."""
    return int(spec.d) - 2 if int(spec.model_id) in (M_HARMONIC_LCD, M_LASCALA_LCD, M_HARMONIC_SDE) else None


def _new_output(shape, device, name=None):
    """Every array a kernel writes its results into is created here and nowhere else, so that a test can substitute the allocator
    (tests/guard_bands.py: outputs embedded in guard bands).  `name`: the array's name in include/chirpgp_hip.h, for such a test's reports."""
    torch = _torch()
    return torch.empty(shape, dtype=torch.float64, device=device)


def _out(t, like_numpy, squeeze):
    if squeeze:
        t = t[0]
    return t.cpu().numpy() if like_numpy else t


class _PerThread(threading.local):
    junction_error = None


_per_thread = _PerThread()


def __getattr__(name):
    # `_engine.last_junction_error`: device tensor [B] of the CALLING THREAD's most recent time-split filter call
    # (cgp_filter_time_split), None when that call fell back to the sequential filter (split_tol) -- the rows returned are then
    # not the split run's.  Prefer `return_junction_error=True`, which hands the tensor back with the results.
    if name == 'last_junction_error':
        return _per_thread.junction_error
    raise AttributeError(name)


def _record_addressing(R, trials_per_record, record_index):
    """The shared-record addressing of include/chirpgp_hip.h (cgp_filter) over R records: -> (ys_repeat, the int32 record numbers
    for ys_index or None, B)."""
    rep = 1 if trials_per_record is None else int(trials_per_record)
    if rep < 1:
        raise ValueError('trials_per_record must be >= 1')
    idx_h = None
    if record_index is not None:
        idx_h = np.ascontiguousarray(np.asarray(record_index, dtype=np.int64).reshape(-1))
        if idx_h.size and (idx_h.min() < 0 or idx_h.max() >= R):
            raise ValueError(f'record_index outside 0..{R - 1}')
        idx_h = idx_h.astype(np.int32)
    return rep, idx_h, (R if idx_h is None else int(idx_h.size)) * rep


def _missing_flag(missing):
    """``missing`` of the filters -> flag bits: None / 'propagate' (the reference: a NaN measurement poisons the state) or 'skip'."""
    if missing is None or missing == 'propagate':
        return 0
    if missing == 'skip':
        return SKIP_MISSING
    raise ValueError(f"missing must be None, 'propagate' or 'skip', not {missing!r}")


def rk4_substeps(n):
    """CGP_RK4_SUBSTEPS(n) of include/chirpgp_hip.h: the flag bits of n = 1 .. 16 RK4 substeps between measurements (n = 1: none)."""
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_SUBSTEPS:
        raise ValueError(f'substeps must be an integer in 1 .. {MAX_SUBSTEPS}, not {n!r}')
    return (int(n) - 1) << 16


def _substeps_flag(substeps, continuous_discrete, time_split, what):
    """``substeps`` of the continuous-discrete methods -> flag bits; what cannot take them is refused here, before anything is launched."""
    bits = rk4_substeps(substeps)
    if bits and not continuous_discrete:
        raise ValueError(f'substeps goes with the continuous-discrete methods only (cd_ekf, cd_eks, cd_sgp_filter, cd_sgp_smoother), not with {what}')
    if bits and time_split is not None:
        raise ValueError('substeps does not go with time_split: the time-split kernels take one RK4 step per sample')
    return bits


def _leading_shape(x):
    return tuple(int(v) for v in (x.shape if hasattr(x, 'shape') else np.shape(x)))


def check_intervals(dts, T, grids=None):
    """``dts`` of a timed call (include/chirpgp_hip_timed.h) -> its host copy, float64 (G, T): (T,) is one time grid for the whole call
    (G = 1), (G, T) one per record -- G must then be ``grids`` where that is given.  A NaN, an infinite or a negative entry is a
    ValueError that names the first one: the C entry points do not look at device memory and would integrate it."""
    a = dts.detach().cpu().numpy() if _is_torch(dts) else np.asarray(dts)
    a = np.ascontiguousarray(a, dtype=np.float64)
    one = a.ndim == 1
    if one:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] != T:
        raise ValueError(f'dts must be (T,) or (records, T) with T = {T}, got {tuple(np.shape(dts))}')
    if not one and grids is not None and a.shape[0] != grids:
        raise ValueError(f'dts has {a.shape[0]} time grids for {grids} records: pass (T,) for one shared grid or one row per record')
    bad = ~(np.isfinite(a) & (a >= 0.0))
    if bad.any():
        g, t = (int(v) for v in np.argwhere(bad)[0])
        where = f'dts[{t}]' if one else f'dts[{g}, {t}]'
        raise ValueError(f'{where} = {float(a[g, t])!r}: an interval must be finite and >= 0 (0: two samples at one instant)')
    return a


def _intervals(dts, T, grids=None, check=True):
    """The intervals of a launch -> (number of grids, the checked host copy or None).  check=False: shapes only -- for a caller that checked
    the same intervals once already (an MLE search passes one grid to every launch; checking a device tensor costs a copy to the host)."""
    if check:
        a = check_intervals(dts, T, grids)
        return a.shape[0], a
    shape = _leading_shape(dts)
    if len(shape) not in (1, 2) or shape[-1] != T or (len(shape) == 2 and grids is not None and shape[0] != grids):
        check_intervals(dts, T, grids)                  # (raises the shape's ValueError)
    return (1 if len(shape) == 1 else shape[0]), None


def _timed_call(dts, dt, continuous_discrete, time_split, what):
    """The refusals of ``dts=`` that need no data: with it dt must be None, the method continuous-discrete, and no time split."""
    if dt is not None:
        raise ValueError('pass either dt or dts=, not both: with dts= every step has its own interval and dt must be None')
    if not continuous_discrete:
        raise ValueError(f'dts= goes with the continuous-discrete methods only (cd_ekf, cd_eks, cd_sgp_filter, cd_sgp_smoother), not with {what}: '
                         f'a discrete model\'s constants are fixed per dt when it is built')
    if time_split is not None:
        raise ValueError('dts= does not go with time_split: there is no timed form of the time-split kernels')


def run_filter(method, spec, sgps, gamma, H, Xi, m0, P0, dt, ys, nll_final_only=False, flags=0, want=(True, True, True),
               trials_per_record=None, record_index=None, time_split=None, split_tol=None, return_junction_error=False, missing=None,
               substeps=1, dts=None, check_dts=True):
    """cgp_filter with NumPy / torch marshalling.  ys (T,) or (B, T) -> (mfs, Pfs, nll) with matching leading axes.

    Shared records (include/chirpgp_hip.h, cgp_filter): with ``trials_per_record = k`` every record of ys -- (T,) or (R, T) --
    serves k consecutive trials (k parameter vectors of a sweep, the 2 P + 1 probes of a difference gradient), B = R k, and
    the results always carry the batch axis; ``record_index`` (n,) picks and orders the records first (B = n k).  The
    record is read from ONE copy in HBM: nothing is replicated.

    ``time_split = (segments, burn_in)``: the time-split filter with burn-in (include/chirpgp_hip.h, cgp_filter_time_split) -- several
    wavefronts per trial for batches that leave most SIMDs idle.  With ``return_junction_error=True`` the per-trial junction mismatch
    of THIS call comes back as a fourth output (device tensor [B]; None if the results are the sequential filter's); it is also
    left, per calling thread, in ``_engine.last_junction_error``.  With ``split_tol`` the call checks it (one device
    synchronisation) and falls back to the sequential filter if any junction is further off.

    ``missing='skip'`` (include/chirpgp_hip.h, CGP_SKIP_MISSING): a NaN measurement is a missing sample -- the prediction is that step's
    filtering result and its NLL increment is exactly 0 -- instead of the reference's poison (None / 'propagate').  Not with
    ``time_split``.

    ``substeps=n`` (include/chirpgp_hip.h, CGP_RK4_SUBSTEPS; cd_ekf and cd_sgp_filter): n = 1 .. 16 RK4 steps of dt / n between two
    measurements instead of one of dt -- the rows n - 1, 2 n - 1, ... of the same filter at step dt / n on the record refined n times
    with gaps at the inserted times, without the n-fold record and outputs.  Not with ``time_split``.

    ``dts=`` (include/chirpgp_hip_timed.h, cgp_filter_timed; cd_ekf and cd_sgp_filter): one interval per step in place of ``dt``, which must
    then be None -- dts[t] is the time from sample t - 1 to sample t, dts[0] from (m0, P0) to sample 0; (T,) is one time grid for the whole
    call, (R, T) one per record of ys, addressed like the records (``trials_per_record``, ``record_index``).  Entries must be finite and
    >= 0 (``check_dts=False``: the caller has checked them, as mle does once per search).  Composes with ``missing`` and ``substeps``; not
    with ``time_split``."""
    n_grids = dts_h = None
    if dts is not None:
        _timed_call(dts, dt, int(method) in (F_CD_EKF, F_CD_SGP), time_split, 'a discrete filter')
        shape = _leading_shape(ys)
        if len(shape) not in (1, 2):
            raise ValueError(f'ys must be (T,) or (B, T), got {shape}')
        n_grids, dts_h = _intervals(dts, shape[-1], shape[0] if len(shape) == 2 else 1, check_dts)
    gaps = _missing_flag(missing)
    if gaps and time_split is not None:
        raise ValueError("missing='skip' does not go with time_split: a burn-in that starts inside a gap has no junction to compare")
    gaps |= _substeps_flag(substeps, int(method) in (F_CD_EKF, F_CD_SGP), time_split, 'a discrete filter')
    junction = None
    torch = _torch()
    like_numpy = not _is_torch(ys)
    ys_d = dev(ys)
    shared = trials_per_record is not None or record_index is not None
    squeeze = ys_d.ndim == 1 and not shared
    if ys_d.ndim == 1:
        ys_d = ys_d[None, :]
    if ys_d.ndim != 2:
        raise ValueError(f'ys must be (T,) or (B, T), got {tuple(ys_d.shape)}')
    T = int(ys_d.shape[1])
    rep, idx_h, B = _record_addressing(int(ys_d.shape[0]), trials_per_record, record_index)
    d = _check_dimension(spec)
    # constants, stream, outputs and the launch all belong to the device the data lives on, whatever the current one is
    with torch.cuda.device(ys_d.device):
        ctx = context(ys_d.device.index)
        keep = [ys_d]
        idx_d = _index_const(idx_h) if idx_h is not None else None
        keep.append(idx_d)
        model = _model_struct(spec, gamma, B, keep)
        sig = _sigma_struct(sgps, d, keep, _nonlinear_coord(spec))
        init = _init_struct(H, Xi, m0, P0, d, B, keep)
        mfs = _new_output((B, T, d), ys_d.device, 'mfs') if want[0] else None
        Pfs = _new_output((B, T, d, d), ys_d.device, 'Pfs') if want[1] else None
        nll = _new_output((B,) if nll_final_only else (B, T), ys_d.device, 'nll') if want[2] else None
        fl = int(flags) | (NLL_FINAL_ONLY if nll_final_only else 0) | gaps
        lib, st = load_library(), _stream()
        if n_grids is not None:
            dts_d = dev(dts, ys_d.device) if _is_torch(dts) else dev_const(dts if dts_h is None else dts_h)      # (cached by value: an MLE search passes one grid again and again)
            keep.append(dts_d)
            rc = _timed('filter', lambda: lib.cgp_filter_timed(ctx, int(method), C.byref(model), C.byref(sig) if sig is not None else None,
                                                               C.byref(init), _ptr(dts_d), T if n_grids > 1 else 0, _ptr(ys_d), T, rep,
                                                               _ptr(idx_d), B, T, _ptr(mfs), _ptr(Pfs), _ptr(nll), fl, st))
            _check(ctx, rc, 'cgp_filter_timed')
            _per_thread.junction_error = None
            return tuple(None if t is None else _out(t, like_numpy, squeeze) for t in (mfs, Pfs, nll))
        if time_split is not None:
            segments, burn_in = (int(v) for v in time_split)
            err = _new_output((B,), ys_d.device, 'junction_err')
            rc = _timed('filter', lambda: lib.cgp_filter_time_split(ctx, int(method), C.byref(model), C.byref(sig) if sig is not None else None,
                                                                    C.byref(init), float(dt), _ptr(ys_d), T, rep, _ptr(idx_d), B, T,
                                                                    _ptr(mfs), _ptr(Pfs), _ptr(nll), fl, segments, burn_in, _ptr(err), st))
            _check(ctx, rc, 'cgp_filter_time_split')
            junction = err
            if split_tol is not None and not bool((err <= float(split_tol)).all()):      # NaN / inf / too far: the sequential filter
                time_split, junction = None, None
        if time_split is None:
            rc = _timed('filter', lambda: lib.cgp_filter(ctx, int(method), C.byref(model), C.byref(sig) if sig is not None else None,
                                                         C.byref(init), float(dt), _ptr(ys_d), T, rep, _ptr(idx_d), B, T,
                                                         _ptr(mfs), _ptr(Pfs), _ptr(nll), fl, st))
            _check(ctx, rc, 'cgp_filter')
        _per_thread.junction_error = junction
        res = tuple(None if t is None else _out(t, like_numpy, squeeze) for t in (mfs, Pfs, nll))
        return res + (junction,) if return_junction_error else res


# ---- models compiled at run time (include/chirpgp_hip.h: cgp_model_from_source) ----------------------------------------------------
_custom_cache = {}


def custom_model(spec, device_index=None):
    """The compiled form of a models.CustomDiscrete / CustomDrift on a device: built by hiprtc on first use (about a second), then cached by
    (device, kind, d, source).  A source that does not compile raises RuntimeError with the compiler's messages."""
    torch = _torch()
    if device_index is None:
        device_index = torch.cuda.current_device()
    key = (device_index, int(spec.kind), int(spec.d), spec.source)
    h = _custom_cache.get(key)
    if h is None:
        ctx = context(device_index)
        h = _vp()
        rc = load_library().cgp_model_from_source(ctx, int(spec.kind), int(spec.d), spec.source.encode(), os.path.join(_HERE, 'csrc').encode(), C.byref(h))
        _check(ctx, rc, 'cgp_model_from_source')
        _custom_cache[key] = h
    return h


def release_custom_models():
    """Unload every runtime-compiled model of this process (cgp_custom_model_destroy: the code objects stay loaded for the life of the process
    otherwise -- a sweep over many sources would accumulate them).  The streams that used them must have drained: synchronises first."""
    if not _custom_cache:
        return 0
    _torch().cuda.synchronize()
    lib = load_library()
    n = len(_custom_cache)
    for h in _custom_cache.values():
        lib.cgp_custom_model_destroy(h)
    _custom_cache.clear()
    return n


def _custom_substeps_flag(spec, substeps):
    """``substeps`` of a run-time compiled model -> flag bits: an SDE model's (models.custom_sde) alone, checked before anything is compiled."""
    bits = rk4_substeps(substeps)
    if bits and int(getattr(spec, 'kind', -1)) != 1:          # include/chirpgp_hip.h: CGP_CUSTOM_SDE
        raise ValueError('substeps goes with the continuous-discrete methods only (a custom_sde model): a discrete model has no ODE to integrate')
    return bits


def run_filter_custom(spec, gamma, H, Xi, m0, P0, dt, ys, nll_final_only=False, want=(True, True, True), flags=0, sgps=None, missing=None,
                      substeps=1):
    """ekf / cd_ekf -- with `sgps`: sgp_filter / cd_sgp_filter -- on a model compiled at run time (cgp_filter_custom): the generic
    one-lane-per-trial kernel instantiated on the caller's source.  ys (T,) or (B, T).  ``missing`` and ``substeps`` (cd_ekf, cd_sgp_filter) as in run_filter."""
    gaps = _missing_flag(missing) | _custom_substeps_flag(spec, substeps)
    torch = _torch()
    like_numpy = not _is_torch(ys)
    ys_d = dev(ys)
    squeeze = ys_d.ndim == 1
    if squeeze:
        ys_d = ys_d[None, :]
    B, T = int(ys_d.shape[0]), int(ys_d.shape[1])
    d = int(spec.d)
    with torch.cuda.device(ys_d.device):
        ctx = context(ys_d.device.index)
        handle = custom_model(spec, ys_d.device.index)
        keep = [ys_d]
        params, pstride, g, gstride = _model_operands(spec, gamma, B, keep)
        sig = _sigma_struct(sgps, d, keep, None)
        init = _init_struct(H, Xi, m0, P0, d, B, keep)
        mfs = _new_output((B, T, d), ys_d.device, 'mfs') if want[0] else None
        Pfs = _new_output((B, T, d, d), ys_d.device, 'Pfs') if want[1] else None
        nll = _new_output((B,) if nll_final_only else (B, T), ys_d.device, 'nll') if want[2] else None
        fl = int(flags) | (NLL_FINAL_ONLY if nll_final_only else 0) | gaps
        rc = _timed('filter', lambda: load_library().cgp_filter_custom(ctx, handle, C.byref(sig) if sig is not None else None, _ptr(params), pstride, _ptr(g), gstride, C.byref(init), float(dt),
                                                                       _ptr(ys_d), T, 1, None, B, T, _ptr(mfs), _ptr(Pfs), _ptr(nll), fl, _stream()))
        _check(ctx, rc, 'cgp_filter_custom')
        return tuple(None if t is None else _out(t, like_numpy, squeeze) for t in (mfs, Pfs, nll))


def run_smoother_custom(spec, gamma, dt, mfs, Pfs, flags=0, sgps=None, substeps=1):
    """eks / cd_eks -- with `sgps`: sgp_smoother / cd_sgp_smoother -- on a model compiled at run time (cgp_smoother_custom).  ``substeps`` (cd_eks,
    cd_sgp_smoother) as in run_smoother: that launch runs one wavefront per trial."""
    flags = int(flags) | _custom_substeps_flag(spec, substeps)
    torch = _torch()
    like_numpy = not _is_torch(mfs)
    m, P = dev(mfs), dev(Pfs)
    squeeze = m.ndim == 2
    if squeeze:
        m, P = m[None], P[None]
    if m.ndim != 3 or P.ndim != 4 or P.shape[:2] != m.shape[:2] or P.shape[2] != m.shape[2] or P.shape[3] != m.shape[2]:
        raise ValueError(f'mfs / Pfs must be (B, T, d) / (B, T, d, d); got {tuple(m.shape)} / {tuple(P.shape)}')
    B, T, d = (int(v) for v in m.shape)
    if d != int(spec.d):
        raise ValueError(f'model dimension {spec.d} != data dimension {d}')
    with torch.cuda.device(m.device):
        ctx = context(m.device.index)
        handle = custom_model(spec, m.device.index)
        keep = [m, P]
        params, pstride, g, gstride = _model_operands(spec, gamma, B, keep)
        sig = _sigma_struct(sgps, d, keep, None)
        mss, Pss = _new_output(tuple(m.shape), m.device, 'mss'), _new_output(tuple(P.shape), P.device, 'Pss')
        rc = _timed('smoother', lambda: load_library().cgp_smoother_custom(ctx, handle, C.byref(sig) if sig is not None else None, _ptr(params), pstride, _ptr(g), gstride, float(dt), _ptr(m), _ptr(P),
                                                                           B, T, _ptr(mss), _ptr(Pss), int(flags), _stream()))
        _check(ctx, rc, 'cgp_smoother_custom')
        return _out(mss, like_numpy, squeeze), _out(Pss, like_numpy, squeeze)


DIR_DOUBLES = 24        # include/chirpgp_hip.h: CGP_DIR_DOUBLES
CD_DIR_DOUBLES = 27     # include/chirpgp_hip.h: CGP_CD_DIR_DOUBLES
FISHER_MAX_DIR = 16     # include/chirpgp_hip.h: CGP_FISHER_MAX_DIR


def run_ekf_nll_grad(spec, H, Xi, m0, P0, dt, ys, dirs, trials_per_record=None, record_index=None, missing=None):
    """cgp_ekf_nll_grad: the EKF's final NLL and its derivative along `dirs` (B, n_dir, 24) -- forward tangents through the scan, one
    launch.  ys (T,) or (R, T) with the shared-record addressing of run_filter.  Returns (nll (B,), grad (B, n_dir)) as device tensors.
    ``missing='skip'`` (CGP_SKIP_MISSING, here and in the three entry points below): a NaN measurement is a missing sample -- the step adds
    exactly nothing to nll, grad and fisher -- instead of the poison it is by default (None / 'propagate')."""
    return _run_nll_grad(spec, None, False, H, Xi, m0, P0, dt, ys, dirs, trials_per_record, record_index, missing)


def run_sgp_nll_grad(spec, sgps, H, Xi, m0, P0, dt, ys, dirs, trials_per_record=None, record_index=None, missing=None):
    """cgp_sgp_nll_grad: the sigma-point filter's final NLL and its derivative along `dirs` (B, n_dir, 24), any d = 4 SigmaPoints `sgps`
    -- forward tangents through the scan, one launch; arguments and results as run_ekf_nll_grad.  The kernel sums over the points
    literally, so the set goes over ungrouped."""
    return _run_nll_grad(spec, _need_sigma(sgps, 'cgp_sgp_nll_grad'), False, H, Xi, m0, P0, dt, ys, dirs, trials_per_record, record_index, missing)


def run_ekf_nll_fisher(spec, H, Xi, m0, P0, dt, ys, dirs, trials_per_record=None, record_index=None, missing=None):
    """cgp_ekf_nll_fisher: run_ekf_nll_grad's results and the Fisher information of the EKF's Gaussian innovations model along `dirs`
    (B, n_dir <= 16, 24), sum_t (d nu_i d nu_j / S + d S_i d S_j / (2 S^2)) -- one launch.  Returns (nll (B,), grad (B, n_dir),
    fisher (B, n_dir, n_dir)) as device tensors."""
    return _run_nll_grad(spec, None, True, H, Xi, m0, P0, dt, ys, dirs, trials_per_record, record_index, missing)


def run_sgp_nll_fisher(spec, sgps, H, Xi, m0, P0, dt, ys, dirs, trials_per_record=None, record_index=None, missing=None):
    """cgp_sgp_nll_fisher: the same for the sigma-point filter, any d = 4 SigmaPoints `sgps`; arguments and results as run_ekf_nll_fisher."""
    return _run_nll_grad(spec, _need_sigma(sgps, 'cgp_sgp_nll_fisher'), True, H, Xi, m0, P0, dt, ys, dirs, trials_per_record, record_index, missing)


def run_cd_ekf_nll_grad(spec, gamma, H, Xi, m0, P0, dt, ys, dirs, trials_per_record=None, record_index=None, missing=None, substeps=1):
    """cgp_cd_ekf_nll_grad: the continuous-discrete EKF's final NLL and its derivative along `dirs` (B, n_dir, 27) -- forward tangents
    through the RK4 stages and the update, one launch.  `spec` the drift's descriptor, `gamma` = b b^T (4, 4) or (B, 4, 4); everything
    else, and the results, as run_ekf_nll_grad.  ``substeps=n``: as run_filter's (the directions do not depend on dt: the same `dirs`)."""
    if gamma is None:
        raise ValueError('cgp_cd_ekf_nll_grad needs gamma = b b^T')
    return _run_nll_grad(spec, None, False, H, Xi, m0, P0, dt, ys, dirs, trials_per_record, record_index, missing, gamma=gamma,
                         flags=rk4_substeps(substeps))


def run_cd_sgp_nll_grad(spec, gamma, sgps, H, Xi, m0, P0, dt, ys, dirs, trials_per_record=None, record_index=None, missing=None, substeps=1):
    """cgp_sgp_nll_grad with the SDE model: the continuous-discrete sigma-point filter's final NLL and its derivative along `dirs`
    (B, n_dir, 27) -- forward tangents through the RK4 stages of the sigma-point moment ODE and the update, one launch (one per 16
    directions).  `spec` the drift's descriptor, `gamma` = b b^T (4, 4) or (B, 4, 4), any d = 4 SigmaPoints `sgps`; everything else, and
    the results, as run_cd_ekf_nll_grad."""
    if gamma is None:
        raise ValueError('cgp_sgp_nll_grad on an SDE model needs gamma = b b^T')
    return _run_nll_grad(spec, _need_sigma(sgps, 'cgp_sgp_nll_grad'), False, H, Xi, m0, P0, dt, ys, dirs, trials_per_record, record_index, missing,
                         gamma=gamma, flags=rk4_substeps(substeps))


def _need_sigma(sgps, entry):
    if sgps is None:
        raise ValueError(f'{entry} needs a sigma-point set')
    return sgps


def _run_nll_grad(spec, sgps, fisher, H, Xi, m0, P0, dt, ys, dirs, trials_per_record, record_index, missing=None, gamma=None, flags=0):
    """The tangent entry points: the sigma-point filter's with `sgps`, the EKF's with None, the continuous-discrete forms of either with
    `gamma` (b b^T; directions of 27 doubles, not 24: cgp_cd_ekf_nll_grad, and cgp_sgp_nll_grad on the SDE model); `fisher`: the matrix as a
    third output; `missing`: as run_filter's, through _missing_flag; `flags`: the bits of CGP_RK4_SUBSTEPS (the continuous-discrete forms)."""
    gaps = _missing_flag(missing) | int(flags)
    torch = _torch()
    ys_d = dev(ys)
    if ys_d.ndim == 1:
        ys_d = ys_d[None, :]
    T = int(ys_d.shape[1])
    rep, idx_h, B = _record_addressing(int(ys_d.shape[0]), trials_per_record, record_index)
    d = _check_dimension(spec)
    # (directions already on the device go over as they are, like ys)
    dirs_h = dirs if _is_torch(dirs) else np.ascontiguousarray(np.asarray(dirs, dtype=np.float64))
    per_dir = DIR_DOUBLES if gamma is None else CD_DIR_DOUBLES
    if dirs_h.ndim != 3 or dirs_h.shape[0] != B or dirs_h.shape[2] != per_dir:
        raise ValueError(f'dirs must be ({B}, n_dir, {per_dir}); got {tuple(dirs_h.shape)}')
    n_dir = int(dirs_h.shape[1])
    with torch.cuda.device(ys_d.device):
        ctx = context(ys_d.device.index)
        idx_d = _index_const(idx_h) if idx_h is not None else None
        keep = [ys_d, idx_d]
        model = _model_struct(spec, gamma, B, keep)
        init = _init_struct(H, Xi, m0, P0, d, B, keep)
        dirs_d = dev(dirs_h, ys_d.device.index)
        outs = ([_new_output((B,), ys_d.device, 'nll'), _new_output((B, n_dir), ys_d.device, 'grad')]
                + ([_new_output((B, n_dir, n_dir), ys_d.device, 'fisher')] if fisher else []))
        entry = f'cgp_{"ekf" if sgps is None else "sgp"}_nll_{"fisher" if fisher else "grad"}' if gamma is None or sgps is not None else 'cgp_cd_ekf_nll_grad'
        sig = [] if sgps is None else [C.byref(_sigma_struct(sgps, d, keep, None))]
        rc = _timed('filter', lambda: getattr(load_library(), entry)(ctx, C.byref(model), *sig, C.byref(init), float(dt), _ptr(ys_d), T, rep, _ptr(idx_d),
                                                                     B, T, _ptr(dirs_d), n_dir, *(_ptr(o) for o in outs), gaps, _stream()))
        _check(ctx, rc, entry)
        return tuple(outs)


E_UNSUPPORTED = -2
_FUNCS = {'softplus': 0, 'g': 0, 'exp': 1, 'identity': 2, 'square': 3}
_gh_cache = {}


def _gh_rule(order):
    """Nodes and weights of the reference's 1-D Gauss-Hermite rule (SigmaPoints.gauss_hermite(1, order), quadratures.py:156-196)."""
    if order not in _gh_cache:
        from chirpgp_amd.quadratures import SigmaPoints
        sg = SigmaPoints.gauss_hermite(1, order)
        _gh_cache[order] = (np.asarray(sg.xi, dtype=np.float64).reshape(-1), np.asarray(sg.w, dtype=np.float64).reshape(-1))
    return _gh_cache[order]


class SmootherSelection(dict):
    """The selected outputs of a smoother call: keys 'mean', 'var', 'expect' (those that were asked for), each (T,) or (B, T)."""
    __getattr__ = dict.get


def run_smoother(method, spec, sgps, gamma, dt, mfs, Pfs, flags=0, want=(True, True), select=None, time_split=None, split_tol=None,
                 return_junction_error=False, substeps=1, dts=None, trials_per_record=None, record_index=None, check_dts=True):
    """cgp_smoother / cgp_smoother_select with NumPy / torch marshalling.  (T, d) / (T, d, d) or with a leading batch axis.

    ``select = dict(comp=k, mean=True, var=True, expect='softplus' | 'exp' | 'identity' | 'square' | None, order=10)`` asks the launch
    for the smoothed marginal of state component k as well: its mean mss[..., k], its variance Pss[..., k, k] and / or E[f(V)] by 1-D
    Gauss-Hermite (quadratures.py:234-274 -- the step behind the smoother in every driver of the reference, demos/ekfs_mle.py:69-77).
    The call then returns ``(mss, Pss, selection)``; with ``want=(False, False)`` the full rows are not written at all (None in their
    place) and a d = 4 smoother moves 8 - 24 bytes a step instead of 160 (include/chirpgp_hip.h: cgp_smoother_select).

    ``substeps=n`` (CGP_RK4_SUBSTEPS; cd_eks and cd_sgp_smoother, on the rows of a filter run with the same n): n backward RK4 steps of
    dt / n per interval, each against the moments the filter's forward substeps passed through.  Not with ``time_split``.

    ``dts=`` (include/chirpgp_hip_timed.h, cgp_smoother_timed; cd_eks and cd_sgp_smoother, on the rows of a filter run with the same
    intervals): one interval per step in place of ``dt``, which must then be None; the step from row t + 1 to row t runs over dts[t + 1].
    (T,) is one time grid for the whole call, (R, T) one per record: without further arguments one per trial, with
    ``trials_per_record`` / ``record_index`` addressed as the filter addressed its records.  ``select`` and ``want`` work as without."""
    n_grids = dts_h = grid_rep = grid_idx = None
    if dts is not None:
        _timed_call(dts, dt, int(method) in (S_CD_EKS, S_CD_SGP), time_split, 'a discrete smoother')
        shape = _leading_shape(mfs)
        if len(shape) not in (2, 3):
            raise ValueError(f'mfs must be (T, d) or (B, T, d), got {shape}')
        n_grids, dts_h = _intervals(dts, shape[-2], None, check_dts)
        grid_rep, grid_idx, grid_B = _record_addressing(n_grids, trials_per_record, record_index)
        n_trials = shape[0] if len(shape) == 3 else 1
        if n_grids > 1 or trials_per_record is not None or record_index is not None:
            if grid_B != n_trials:
                raise ValueError(f'dts addresses {grid_B} trials, mfs has {n_trials}')
    elif trials_per_record is not None or record_index is not None:
        raise ValueError('trials_per_record / record_index address the time grids of dts=')
    flags = int(flags) | _substeps_flag(substeps, int(method) in (S_CD_EKS, S_CD_SGP), time_split, 'a discrete smoother')
    torch = _torch()
    like_numpy = not _is_torch(mfs)
    m, P = dev(mfs), dev(Pfs)
    squeeze = m.ndim == 2
    if squeeze:
        m, P = m[None], P[None]
    if m.ndim != 3 or P.ndim != 4 or P.shape[:2] != m.shape[:2] or P.shape[2] != m.shape[2] or P.shape[3] != m.shape[2]:
        raise ValueError(f'mfs / Pfs must be (B, T, d) / (B, T, d, d); got {tuple(m.shape)} / {tuple(P.shape)}')
    B, T, d = (int(s) for s in m.shape)
    if d != int(spec.d):
        raise ValueError(f'model dimension {spec.d} != data dimension {d}')
    _check_dimension(spec)
    if select is None and not (want[0] and want[1]):
        raise ValueError('a smoother without `select` writes both mss and Pss')
    with torch.cuda.device(m.device):
        ctx = context(m.device.index)
        keep = [m, P]
        model = _model_struct(spec, gamma, B, keep)
        sig = _sigma_struct(sgps, d, keep, _nonlinear_coord(spec))
        lib, st = load_library(), _stream()
        sig_ref = C.byref(sig) if sig is not None else None
        # the launch: cgp_smoother / cgp_smoother_select with dt, or cgp_smoother_timed -- one entry point for both -- with the intervals
        smooth_full = lambda mss_, Pss_: lib.cgp_smoother(ctx, int(method), C.byref(model), sig_ref, float(dt), _ptr(m), _ptr(P), B, T,      # noqa: E731
                                                          _ptr(mss_), _ptr(Pss_), int(flags), st)
        smooth_select = lambda o_: lib.cgp_smoother_select(ctx, int(method), C.byref(model), sig_ref, float(dt), _ptr(m), _ptr(P), B, T,      # noqa: E731
                                                           C.byref(o_), int(flags), st)
        entry_full, entry_select = 'cgp_smoother', 'cgp_smoother_select'
        if n_grids is not None:
            dts_d = dev(dts, m.device) if _is_torch(dts) else dev_const(dts if dts_h is None else dts_h)
            gidx_d = _index_const(grid_idx) if grid_idx is not None else None
            keep += [dts_d, gidx_d]
            shared_grid = n_grids == 1 and grid_idx is None and trials_per_record is None

            def smooth_select(o_):
                return lib.cgp_smoother_timed(ctx, int(method), C.byref(model), sig_ref, _ptr(dts_d), 0 if shared_grid else T,
                                              1 if shared_grid else grid_rep, _ptr(gidx_d), _ptr(m), _ptr(P), B, T, C.byref(o_), int(flags), st)

            def smooth_full(mss_, Pss_):
                o_ = CgpSmoothOut()
                o_.mss, o_.Pss, o_.comp = _ptr(mss_), _ptr(Pss_), -1
                return smooth_select(o_)
            entry_full = entry_select = 'cgp_smoother_timed'
        if time_split is not None:
            # cgp_smoother_time_split (cd_sgp_smoother, cd_eks): several wavefronts per trial, each starting `burn_in` steps later than its piece from the
            # filtering row there; the launch reports the mismatch at its junctions (with split_tol: fall back to the sequential smoother)
            if select is not None:
                raise ValueError('time_split writes full rows only')
            segments, burn_in = (int(v) for v in time_split)
            mss, Pss = _new_output(tuple(m.shape), m.device, 'mss'), _new_output(tuple(P.shape), P.device, 'Pss')
            err = _new_output((B,), m.device, 'junction_err')
            rc = _timed('smoother', lambda: lib.cgp_smoother_time_split(ctx, int(method), C.byref(model), sig_ref, float(dt), _ptr(m), _ptr(P), B, T,
                                                                        _ptr(mss), _ptr(Pss), int(flags), segments, burn_in, _ptr(err), st))
            _check(ctx, rc, 'cgp_smoother_time_split')
            junction = err
            if split_tol is not None and not bool((err <= float(split_tol)).all()):
                rc = _timed('smoother', lambda: lib.cgp_smoother(ctx, int(method), C.byref(model), sig_ref, float(dt), _ptr(m), _ptr(P), B, T,
                                                                 _ptr(mss), _ptr(Pss), int(flags), st))
                _check(ctx, rc, 'cgp_smoother')
                junction = None
            _per_thread.junction_error = junction
            res = (_out(mss, like_numpy, squeeze), _out(Pss, like_numpy, squeeze))
            return res + (junction,) if return_junction_error else res
        if select is None:
            mss, Pss = _new_output(tuple(m.shape), m.device, 'mss'), _new_output(tuple(P.shape), P.device, 'Pss')
            rc = _timed('smoother', lambda: smooth_full(mss, Pss))
            _check(ctx, rc, entry_full)
            return _out(mss, like_numpy, squeeze), _out(Pss, like_numpy, squeeze)
        unknown = set(select) - {'comp', 'mean', 'var', 'expect', 'order'}
        if unknown:
            raise ValueError(f'select: unknown keys {sorted(unknown)}')
        comp = int(select['comp'])
        if comp < 0:
            comp += d                                   # "-2": the frequency state of every chirp model
        if not 0 <= comp < d:
            raise ValueError(f'select: component {select["comp"]} outside the state dimension {d}')
        func = select.get('expect')
        if func is not None and func is not False and str(func) not in _FUNCS:
            raise ValueError(f'select: expect must be one of {sorted(_FUNCS)} (an enumerated integrand: a Python callable cannot run in a kernel)')
        want_e = func is not None and func is not False
        order = int(select.get('order', 10))
        o = CgpSmoothOut()
        o.comp, o.func, o.order = comp, (_FUNCS[str(func)] if want_e else 0), order
        sel = {}
        for key, field in (('mean', 'comp_mean'), ('var', 'comp_var')):
            if select.get(key, False):
                sel[key] = _new_output((B, T), m.device, field)
                setattr(o, field, _ptr(sel[key]))
        if want_e:
            xi, w = _gh_rule(order)
            xi_d, w_d = dev_const(xi), dev_const(w)
            keep += [xi_d, w_d]
            sel['expect'] = _new_output((B, T), m.device, 'expect')
            o.expect, o.xi, o.w = _ptr(sel['expect']), _ptr(xi_d), _ptr(w_d)
        if not sel:
            raise ValueError('select asks for none of mean / var / expect')
        mss = _new_output(tuple(m.shape), m.device, 'mss') if want[0] else None
        Pss = _new_output(tuple(P.shape), P.device, 'Pss') if want[1] else None
        o.mss, o.Pss = _ptr(mss), _ptr(Pss)
        rc = _timed('smoother', lambda: smooth_select(o))
        if rc == E_UNSUPPORTED and (mss is None or Pss is None):
            # a kernel that can only gather the selection from its full rows: give it (temporary) rows
            tm = mss if mss is not None else _new_output(tuple(m.shape), m.device, 'mss (temporary)')
            tP = Pss if Pss is not None else _new_output(tuple(P.shape), P.device, 'Pss (temporary)')
            o.mss, o.Pss = _ptr(tm), _ptr(tP)
            rc = _timed('smoother', lambda: smooth_select(o))
            keep += [tm, tP]
        _check(ctx, rc, entry_select)
        selection = SmootherSelection({k: _out(v, like_numpy, squeeze) for k, v in sel.items()})
        return (None if mss is None else _out(mss, like_numpy, squeeze), None if Pss is None else _out(Pss, like_numpy, squeeze), selection)


def run_smoother_sample(method, spec, sgps, dt, mfs, Pfs, n_samples, seed=0, trial0=0, sample0=0, normals=None, want_paths=True, select=None,
                        flags=0):
    """cgp_smoother_sample with NumPy / torch marshalling: ``n_samples`` joint posterior sample paths per trial by backward simulation on the
    discrete smoother's own affine maps (include/chirpgp_hip.h).  mfs / Pfs are (T, d) / (T, d, d) or carry a leading batch axis, and are
    taken as run_smoother takes them (float64, contiguous, on the GPU -- converted where they are not).

    ``normals`` None: the engine's Philox stream, addressed by (seed, trial0 + b, sample0 + s, step) alone -- a path does not depend on the
    batch, on n_samples or on how trials and samples are split over calls.  Otherwise the caller's standard normals, (B, S, T, d) ((S, T, d)
    without the batch axis).  ``select = dict(comp=k, func='softplus' | 'exp' | 'identity' | 'square')`` asks for func(x[comp]) of every sample
    and step.  Returns ``(paths | None, comp_paths | None)``: (B, S, T, d) and (B, S, T), without B for unbatched rows."""
    torch = _torch()
    like_numpy = not _is_torch(mfs)
    m, P = dev(mfs), dev(Pfs)
    squeeze = m.ndim == 2
    if squeeze:
        m, P = m[None], P[None]
    if m.ndim != 3 or P.ndim != 4 or P.shape[:2] != m.shape[:2] or P.shape[2] != m.shape[2] or P.shape[3] != m.shape[2]:
        raise ValueError(f'mfs / Pfs must be (B, T, d) / (B, T, d, d); got {tuple(m.shape)} / {tuple(P.shape)}')
    B, T, d = (int(v) for v in m.shape)
    S = int(n_samples)
    if S < 0:
        raise ValueError('n_samples must be >= 0')
    if d != int(spec.d):
        raise ValueError(f'model dimension {spec.d} != data dimension {d}')
    _check_dimension(spec)
    if not want_paths and select is None:
        raise ValueError('nothing to write: want_paths=False needs select=dict(comp=..., func=...)')
    o = CgpSampleOut()
    if select is not None:
        unknown = set(select) - {'comp', 'func'}
        if unknown:
            raise ValueError(f'select: unknown keys {sorted(unknown)}')
        comp = int(select['comp'])
        if comp < 0:
            comp += d
        if not 0 <= comp < d:
            raise ValueError(f'select: component {select["comp"]} outside the state dimension {d}')
        func = str(select.get('func', 'identity'))
        if func not in _FUNCS:
            raise ValueError(f'select: func must be one of {sorted(_FUNCS)} (an enumerated function: a Python callable cannot run in a kernel)')
        o.comp, o.func = comp, _FUNCS[func]
    with torch.cuda.device(m.device):
        ctx = context(m.device.index)
        keep = [m, P]
        z = None
        if normals is not None:
            z = dev(normals, m.device)
            if squeeze and z.ndim == 3:
                z = z[None]
            if tuple(z.shape) != (B, S, T, d):
                raise ValueError(f'normals must be (B, S, T, d) = {(B, S, T, d)}; got {tuple(z.shape)}')
            keep.append(z)
        model = _model_struct(spec, None, B, keep)
        sig = _sigma_struct(sgps, d, keep, _nonlinear_coord(spec))
        paths = _new_output((B, S, T, d), m.device, 'paths') if want_paths else None
        comp_paths = _new_output((B, S, T), m.device, 'comp_paths') if select is not None else None
        o.paths, o.comp_paths = _ptr(paths), _ptr(comp_paths)
        rc = _timed('sample', lambda: load_library().cgp_smoother_sample(ctx, int(method), C.byref(model), C.byref(sig) if sig is not None else None, float(dt),
                                                                         _ptr(m), _ptr(P), B, T, S, int(seed), int(trial0), int(sample0), _ptr(z),
                                                                         C.byref(o), int(flags), _stream()))
        _check(ctx, rc, 'cgp_smoother_sample')
    return (None if paths is None else _out(paths, like_numpy, squeeze), None if comp_paths is None else _out(comp_paths, like_numpy, squeeze))


FN_SOFTPLUS, FN_EXP, FN_IDENTITY, FN_SQUARE = 0, 1, 2, 3


def gaussian_expectation(ms, chol_Ps, xi, w, func=FN_SOFTPLUS):
    """E[f(V)] for scalar marginals on the device (f enumerated: FN_*) -> (n, 1) like the reference's force_shape=True call."""
    torch = _torch()
    like_numpy = not _is_torch(ms)
    m, s = dev(ms).reshape(-1), dev(chol_Ps).reshape(-1)
    if m.shape != s.shape:
        raise ValueError('ms and chol_Ps must have the same number of entries')
    with torch.cuda.device(m.device):
        ctx = context(m.device.index)
        xi_d, w_d = dev(xi).reshape(-1), dev(w).reshape(-1)
        out = _new_output(tuple(m.shape), m.device, 'out')
        rc = load_library().cgp_gaussian_expectation_fn(ctx, int(func), _ptr(m), _ptr(s), m.numel(), 1, _ptr(xi_d), _ptr(w_d), xi_d.numel(),
                                                        _ptr(out), _stream())
        _check(ctx, rc, 'cgp_gaussian_expectation_fn')
        out = out.reshape(-1, 1)
        return out.cpu().numpy() if like_numpy else out


def debug_math(op, x):
    """In-kernel elementary functions on the device (test hook): returns (out0, out1) as NumPy arrays.  The two-argument ops
    (DEBUG_MATH_PAIR_OPS) take x as (n, 2) pairs and return n results."""
    torch = _torch()
    xd = dev(x).reshape(-1)
    with torch.cuda.device(xd.device):
        ctx = context(xd.device.index)
        o0, o1 = torch.empty_like(xd), torch.empty_like(xd)
        rc = load_library().cgp_debug_math(ctx, int(op), _ptr(xd), xd.numel(), _ptr(o0), _ptr(o1), _stream())
        _check(ctx, rc, 'cgp_debug_math')
        keep = xd.numel() // 2 if int(op) in DEBUG_MATH_PAIR_OPS else xd.numel()
        return o0[:keep].cpu().numpy(), o1[:keep].cpu().numpy()


DEBUG_MATH_PAIR_OPS = (22, 23, 25)


def _init_struct(H, Xi, m0, P0, d, B, keep):
    init = CgpInit()
    if H is not None:
        Ht, init.H_stride = _batched_operand(H, 1, B, 'H')
        if Ht.shape[-1] != d:
            raise ValueError(f'H must have {d} entries')
        init.H = _ptr(Ht)
        keep.append(Ht)
    if Xi is not None:
        Xit = dev_const(np.asarray(Xi, dtype=np.float64).reshape(-1)) if not _is_torch(Xi) else dev(Xi.reshape(-1))
        if Xit.numel() not in (1, B):
            raise ValueError('Xi must be a scalar or have one entry per trial')
        init.Xi, init.Xi_stride = _ptr(Xit), (1 if Xit.numel() > 1 else 0)
        keep.append(Xit)
    m0t, init.m0_stride = _batched_operand(m0, 1, B, 'm0')
    if m0t.shape[-1] != d:
        raise ValueError(f'm0 must be ({d},)')
    init.m0 = _ptr(m0t)
    keep.append(m0t)
    if P0 is not None:
        P0t, init.P0_stride = _batched_operand(P0, 2, B, 'P0')
        if tuple(P0t.shape[-2:]) != (d, d):
            raise ValueError(f'P0 must be ({d}, {d})')
        init.P0 = _ptr(P0t)
        keep.append(P0t)
    return init


def run_simulate(spec, H, Xi, m0, P0, dt, T, seed, B, trial0=0, want=(True, True), flags=0, device=None):
    """cgp_simulate: B trajectories xs (B, T, d) and measurements ys (B, T) as CUDA tensors (None where not wanted)."""
    torch = _torch()
    d = _check_dimension(spec)
    B, T = int(B), int(T)
    with torch.cuda.device(torch.cuda.current_device() if device is None else device):
        ctx = context(device)
        keep = []
        model = _model_struct(spec, None, B, keep)
        init = _init_struct(H if want[1] else None, Xi if want[1] else None, m0, P0, d, B, keep)
        on = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        xs = _new_output((B, T, d), on, 'xs') if want[0] else None
        ys = _new_output((B, T), on, 'ys') if want[1] else None
        lib, st = load_library(), _stream()
        fl = int(flags) | (SIM_FIXED_X0 if P0 is None else 0)
        rc = _timed('simulate', lambda: lib.cgp_simulate(ctx, C.byref(model), C.byref(init), float(dt), int(seed) & (2 ** 64 - 1),
                                                         int(trial0), B, T, _ptr(xs), _ptr(ys), fl, st))
        _check(ctx, rc, 'cgp_simulate')
        return xs, ys


def add_noise(clean, Xi, seed, B, trial0=0):
    """cgp_add_noise: (B, T) CUDA tensor clean + sqrt(Xi) e; clean is (T,) (shared) or (B, T)."""
    torch = _torch()
    c = dev(clean)
    if c.ndim == 1:
        stride, T = 0, int(c.shape[0])
    elif c.ndim == 2 and c.shape[0] == B:
        stride, T = int(c.shape[1]), int(c.shape[1])
    else:
        raise ValueError(f'clean must be (T,) or ({B}, T), got {tuple(c.shape)}')
    with torch.cuda.device(c.device):
        Xit = dev_const(np.asarray(Xi, dtype=np.float64).reshape(-1)) if not _is_torch(Xi) else dev(Xi.reshape(-1))
        if Xit.numel() not in (1, B):
            raise ValueError('Xi must be a scalar or have one entry per trial')
        ctx = context(c.device.index)
        ys = _new_output((int(B), T), c.device, 'ys')
        rc = _timed('add_noise', lambda: load_library().cgp_add_noise(ctx, _ptr(c), stride, _ptr(Xit), 1 if Xit.numel() > 1 else 0,
                                                                      int(seed) & (2 ** 64 - 1), int(trial0), int(B), T, _ptr(ys), _stream()))
        _check(ctx, rc, 'cgp_add_noise')
        return ys


def debug_philox(ctr, key):
    """Raw Philox4x32-10 blocks on the device (test hook): ctr (n, 4) uint32, key (2,) uint32 -> (n, 4) uint32."""
    torch = _torch()
    c = torch.from_numpy(np.ascontiguousarray(np.asarray(ctr, dtype=np.uint32)).view(np.int32)).cuda()
    k = torch.from_numpy(np.ascontiguousarray(np.asarray(key, dtype=np.uint32)).view(np.int32)).cuda()
    ctx = context(c.device.index)
    out = torch.empty_like(c)
    rc = load_library().cgp_debug_philox(ctx, _ptr(c), _ptr(k), c.shape[0], _ptr(out), _stream())
    _check(ctx, rc, 'cgp_debug_philox')
    return out.cpu().numpy().view(np.uint32)


DBG_WALK_SEGMENTS, DBG_COUNT_REGIMES, DBG_LANE_BUFFERS = 1, 2, 3
REGIME_COUNTERS = ('high', 'common', 'redone', 'checked', 'high_left', 'wide', 'low', 'mid')


def reserve_workspace(nbytes, device_index=None):
    """Size the current stream's scratch buffer of the time-split launches ahead of time (include/chirpgp_hip.h:
    cgp_reserve_workspace) -- needed only before capturing such launches into a graph."""
    ctx = context(device_index)
    _check(ctx, load_library().cgp_reserve_workspace(ctx, int(nbytes), _stream()), 'cgp_reserve_workspace')


def release_workspace(device_index=None):
    """Free the current stream's scratch buffer and forget the stream (include/chirpgp_hip.h: cgp_release_workspace)."""
    ctx = context(device_index)
    _check(ctx, load_library().cgp_release_workspace(ctx, _stream()), 'cgp_release_workspace')


def debug_set(key, value, device_index=None):
    """Per-context tuning / measurement knob (include/chirpgp_hip.h: cgp_debug_set)."""
    ctx = context(device_index)
    _check(ctx, load_library().cgp_debug_set(ctx, int(key), int(value)), 'cgp_debug_set')


def debug_counters(reset=True, device_index=None):
    """The context's regime counters as a dict (waits for the current stream): chunks of 64 steps the d = 4 matrix-core EKF kept from
    its HIGH / common regime, repeated with the checked step, ran on the checked step afterwards, and tried in HIGH but left it."""
    ctx = context(device_index)
    out = (C.c_uint64 * 8)()
    _check(ctx, load_library().cgp_debug_counters(ctx, out, 1 if reset else 0, _stream()), 'cgp_debug_counters')
    return {k: int(out[i]) for i, k in enumerate(REGIME_COUNTERS)}


def squared_error_sums(a, r, comps, sums=None):
    """sums[c][0][t] += sum_b (a - r)[b, t, comps[c]]^2, sums[c][1][t] += sum_b of its square (include/chirpgp_hip.h:
    cgp_squared_error_sums) -- the per-step error statistics of the reference's CRLB jobs, reduced on the device.  a, r: (B, T, d)
    device tensors; returns the (n, 2, T) tensor of sums (a fresh zeroed one unless `sums` is passed to accumulate into)."""
    torch = _torch()
    a = dev(a)
    r = dev(r, a.device.index)
    if r.device != a.device:
        r = r.to(a.device)
    if a.shape != r.shape or a.ndim != 3:
        raise ValueError(f'a and r must both be (B, T, d); got {tuple(a.shape)}, {tuple(r.shape)}')
    B, T, d = (int(v) for v in a.shape)
    comps = [int(c) for c in comps]
    with torch.cuda.device(a.device):
        ctx = context(a.device.index)
        if sums is None:
            sums = torch.zeros((len(comps), 2, T), dtype=torch.float64, device=a.device)
        elif (not _is_torch(sums) or tuple(sums.shape) != (len(comps), 2, T) or not sums.is_contiguous() or sums.dtype != torch.float64
              or not sums.is_cuda or sums.device != a.device):
            # the kernel adds float64 atomically through the raw pointer: anything else is a wrong result or a fault
            raise ValueError(f'sums must be a contiguous float64 ({len(comps)}, 2, {T}) tensor on {a.device}')
        arr = (C.c_int32 * len(comps))(*comps)
        for lo in range(0, max(B, 1), 65535 * 512):                    # the kernel's grid limit: slabs of 512 trials
            hi = min(B, lo + 65535 * 512)
            rc = load_library().cgp_squared_error_sums(ctx, _ptr(a[lo:hi]), _ptr(r[lo:hi]), hi - lo, T, d, arr, len(comps), _ptr(sums), _stream())
            _check(ctx, rc, 'cgp_squared_error_sums')
    return sums


def pcrlb_rows(d):
    """K = d (d + 1) / 2 + d d: the rows of cgp_pcrlb_sums' output (packed lower triangle of D11, then D12 row-major)."""
    return d * (d + 1) // 2 + d * d


def run_pcrlb_sums(spec, dt, x0, xs, sums=None, flags=0):
    """cgp_pcrlb_sums: the Monte-Carlo sums of the posterior Cramer-Rao recursion's D11 and D12 blocks over the trials of x0 (B, d) and
    xs (B, T, d), added into the (K, T) device tensor `sums` (a fresh zeroed one unless passed) -- include/chirpgp_hip.h."""
    torch = _torch()
    d = _check_dimension(spec)
    xs = dev(xs)
    x0 = dev(x0, xs.device.index)
    if x0.device != xs.device:
        x0 = x0.to(xs.device)
    if xs.ndim != 3 or xs.shape[2] != d or tuple(x0.shape) != (xs.shape[0], d):
        raise ValueError(f'xs must be (B, T, {d}) and x0 (B, {d}); got {tuple(xs.shape)}, {tuple(x0.shape)}')
    B, T = int(xs.shape[0]), int(xs.shape[1])
    K = pcrlb_rows(d)
    with torch.cuda.device(xs.device):
        ctx = context(xs.device.index)
        if sums is None:
            sums = _new_output((K, T), xs.device, 'sums').zero_()
        elif (not _is_torch(sums) or tuple(sums.shape) != (K, T) or not sums.is_contiguous() or sums.dtype != torch.float64
              or not sums.is_cuda or sums.device != xs.device):
            # the kernel adds float64 atomically through the raw pointer: anything else is a wrong result or a fault
            raise ValueError(f'sums must be a contiguous float64 ({K}, {T}) tensor on {xs.device}')
        keep = []
        model = _model_struct(spec, None, 1, keep)
        lib = load_library()
        for lo in range(0, max(B, 1), 65535 * 512):                    # the kernel's grid limit: slabs of 512 trials
            hi = min(B, lo + 65535 * 512)
            rc = _timed('pcrlb_sums', lambda: lib.cgp_pcrlb_sums(ctx, C.byref(model), float(dt), _ptr(x0[lo:hi]), _ptr(xs[lo:hi]), hi - lo, T,
                                                                 _ptr(sums), int(flags), _stream()))
            _check(ctx, rc, 'cgp_pcrlb_sums')
    return sums


def run_simulate_x0(d, m0, P0, seed, B, trial0=0, device=None):
    """cgp_simulate_x0: the (B, d) initial samples x_0 = m0 + chol(P0) z that run_simulate draws for trials trial0 .. trial0 + B - 1."""
    torch = _torch()
    d, B = int(d), int(B)
    if not 1 <= d <= 8:
        raise NotImplementedError(f'state dimension {d} outside 1..8 is not compiled into cgp_simulate_x0')
    with torch.cuda.device(torch.cuda.current_device() if device is None else device):
        ctx = context(device)
        keep = []
        model = CgpModel()
        model.model_id, model.d = M_LINEAR, d
        init = _init_struct(None, None, m0, P0, d, B, keep)
        on = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        x0 = _new_output((B, d), on, 'x0')
        rc = _timed('simulate_x0', lambda: load_library().cgp_simulate_x0(ctx, C.byref(model), C.byref(init), int(seed) & (2 ** 64 - 1), int(trial0), B,
                                                                          _ptr(x0), _stream()))
        _check(ctx, rc, 'cgp_simulate_x0')
        return x0
