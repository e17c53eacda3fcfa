"""The case table of the C-ABI's argument checks (csrc/cgp_args.hpp): per entry point one good call at the smallest shape that reaches
the launch -- B = 1, T = 8, the d = 4 chirp model, the cubature set where a set is needed, n_dir = 6, S = 2, d = 2 for a run-time-compiled
model -- and (label, edit) rows that each make one argument of it faulty, or the call empty.  tests/golden/abi_refusals.json holds what
every row returns: the code and the message.

The arguments of a call are a dict in the order of the C signature: scalars by value, structs as Rec (the fields of the C struct), a
pointer as the NAME of its buffer (None is NULL).  Two users resolve the names: test_abi_refusals.py hands them to the host program
tests/abi_probe.hip as non-null fakes (probe_line), test_gpu_abi_refusals.py allocates the buffers of buffers() on the device and calls
the library (call).  A row marked DERIVED is a limit no device buffer can reach (2^31 trials, a 32-bit counter's worth of steps) or needs
a second device: it is asked of the host program only, and its golden answer is read off the source."""
import ctypes as C
import types

import numpy as np

FILL = 123.0
DERIVED = 'derived'
F_EKF, F_SGP, F_CD_EKF, F_CD_SGP, F_EKF_KPT = range(5)
S_EKS, S_SGP, S_CD_EKS, S_CD_SGP = range(4)
M_LINEAR, M_HARMONIC_LCD, M_LASCALA_LCD, M_LINEAR_SDE, M_HARMONIC_SDE, M_KPT = range(6)
WAVE_PER_TRIAL, THREAD_PER_TRIAL, GENERIC_KERNEL, SKIP_MISSING = 0x2, 0x4, 0x10, 0x2000
E_ARG, E_UNSUPPORTED = -1, -2
T, N_DIR, S = 8, 6, 2


class Rec(types.SimpleNamespace):
    """A struct argument: the C struct's fields, pointers as buffer names."""


def lcd():
    return Rec(model_id=M_HARMONIC_LCD, d=4, n_harm=1, n_params=5, params='lcd', param_stride=0, gamma=None, gamma_stride=0)


def sde():
    return Rec(model_id=M_HARMONIC_SDE, d=4, n_harm=1, n_params=3, params='sde', param_stride=0, gamma='gamma', gamma_stride=0)


def cubature(s=8):
    return Rec(s=s, d=4, xi='xi', w='w', group_start=None, n_groups=0, flags=0)


def init(d=4):
    tag = '' if d == 4 else str(d)
    return Rec(H='H' + tag, H_stride=0, Xi='Xi', Xi_stride=0, m0='m0' + tag, m0_stride=0, P0='P0' + tag, P0_stride=0)


def full_select():
    return Rec(mss='mss', Pss='Pss', comp=2, func=0, comp_mean='comp_mean', comp_var='comp_var', expect='expect', xi='ghx', w='ghw', order=3)


def custom():
    """What cgp_filter_custom / cgp_smoother_custom know of the compiled model (cgp_args.hpp: CustomModel).  The device test passes the
    handle of CUSTOM_BODY instead; only `present` counts there."""
    return Rec(present=1, kind=0, d=2, device=0, ekf=1, sgp=1)


CUSTOM_KIND, CUSTOM_D = 0, 2              # CGP_CUSTOM_DISCRETE
CUSTOM_BODY = '''
template <class T> __device__ void cond_mean(const T* u, const double* p, double dt, T* m) { m[0] = p[0] * u[0] + dt * u[1]; m[1] = p[1] * u[1]; }
__device__ void cond_cov(const double* u, const double* p, double dt, double* c) { c[0] = p[2]; c[1] = 0.0; c[2] = 0.0; c[3] = p[2]; }
'''


def _set(**kw):
    return lambda a: a.update({k: Rec(**vars(v)) if isinstance(v, Rec) else v for k, v in kw.items()})


def _field(arg, **kw):
    def edit(a):
        for k, v in kw.items():
            setattr(a[arg], k, v)
    return edit


def _both(*edits):
    def edit(a):
        for e in edits:
            e(a)
    return edit


def _model_d6(a):
    a['model'].d, a['model'].n_harm = 6, 2         # the two-harmonic chirp model


# ---- what the tangent entry points share (test_gpu_tangent_arguments.py): (what is wrong, the edit that makes it so, the code,
# sigma-point entry points only)
TANGENT_FAULTS = [('dirs = NULL', lambda a: a.update(dirs=None), E_ARG, False),
                  ('nll = NULL', lambda a: a.update(nll=None), E_ARG, False),
                  ('grad = NULL', lambda a: a.update(grad=None), E_ARG, False),
                  ('ys_repeat = 0', lambda a: a.update(ys_repeat=0), E_ARG, False),
                  ('ys_stride = -1', lambda a: a.update(ys_stride=-1), E_ARG, False),
                  ('param_stride = 1', lambda a: setattr(a['model'], 'param_stride', 1), E_ARG, False),
                  ('init.P0 = NULL', lambda a: setattr(a['init'], 'P0', None), E_ARG, False),
                  ('a d = 6 model', _model_d6, E_UNSUPPORTED, False),
                  ('a sigma-point set with d = 6', lambda a: setattr(a['sigma'], 'd', 6), E_UNSUPPORTED, True),
                  ('sigma = NULL', lambda a: a.update(sigma=None), E_ARG, True),
                  ('B = 0', lambda a: a.update(B=0), 0, False)]

EMPTY = [('B = 0', _set(B=0)), ('T = 0', _set(T=0))]
# the model checks every enumerated-model entry shares (cgp_args.hpp: check_model), as edits of the d = 4 chirp model
MODEL_FAULTS = [('model = NULL', _set(model=None)),
                ('model.params = NULL', _field('model', params=None)),
                ('model.d = 0', _field('model', d=0)),
                ('model.d = 13', _field('model', d=13)),
                ('model_id = 17', _field('model', model_id=17)),
                ('model.n_params = 4', _field('model', n_params=4)),
                ('model.d = 6', _field('model', d=6)),
                ('model.param_stride = 1', _field('model', param_stride=1))]
SIGMA_FAULTS = [('sigma = NULL', _set(sigma=None)),
                ('sigma.w = NULL', _field('sigma', w=None)),
                ('sigma.d = 6', _field('sigma', d=6)),
                ('sigma.n_groups = 0 with groups', _field('sigma', group_start='xi', n_groups=0))]


def _tangent(entry):
    sgp, fisher, cd = '_sgp_' in entry, entry.endswith('_fisher'), '_cd_' in entry
    good = dict(model=sde() if cd else lcd())
    if sgp:
        good['sigma'] = cubature()
    good.update(init=init(), dt=1e-3, ys='ys', ys_stride=T, ys_repeat=1, ys_index=None, B=1, T=T, dirs='dirs', n_dir=N_DIR, nll='nll1', grad='grad')
    if fisher:
        good['fisher'] = 'fisher'
    good['flags'] = 0
    rows = [(label, edit) for label, edit, _, sigma_only in TANGENT_FAULTS if sgp or not sigma_only]
    rows += [('n_dir = -1', _set(n_dir=-1)), ('n_dir = 0', _set(n_dir=0)), ('model = NULL', _set(model=None)), ('ys = NULL', _set(ys=None)),
             ('init = NULL', _set(init=None)), ('flags = CGP_WAVE_PER_TRIAL', _set(flags=WAVE_PER_TRIAL)),
             ('flags = CGP_SKIP_MISSING | 0x100', _set(flags=SKIP_MISSING | 0x100))]
    if fisher:
        rows += [('n_dir = 17', _set(n_dir=17)), ('fisher = NULL', _set(fisher=None))]
    if sgp:
        rows += [('sigma.xi = NULL', _field('sigma', xi=None)), ('a set of 2000 points', _field('sigma', s=2000)),
                 ('B = 2^31', _set(B=2 ** 31), DERIVED)]
    elif fisher:
        rows += [('B = 10 (2^31 - 1) + 1', _set(B=10 * (2 ** 31 - 1) + 1), DERIVED)]        # 64 / 6 = 10 trials a wavefront
    if cd:
        rows += [('model.gamma = NULL', _field('model', gamma=None)), ('model.gamma_stride = 1', _field('model', gamma_stride=1)),
                 ('a discrete model', _set(model=lcd())), ('B n_dir > 64 (2^31 - 1)', _set(B=(2 ** 31 - 1) * 64 // 6 + 1), DERIVED)]
    return dict(good=good, outputs=('nll1', 'grad') + (('fisher',) if fisher else ()), rows=rows)


_FILTER = dict(method=F_EKF, model=lcd(), sigma=None, init=init(), dt=1e-3, ys='ys', ys_stride=T, ys_repeat=1, ys_index=None, B=1, T=T,
               mfs='mfs_out', Pfs='Pfs_out', nll='nll', flags=0)
_FILTER_ROWS = EMPTY + [('B = -1', _set(B=-1)), ('ys = NULL', _set(ys=None)), ('ys_stride = -1', _set(ys_stride=-1)), ('ys_repeat = 0', _set(ys_repeat=0)),
                        ('init = NULL', _set(init=None)), ('init.P0 = NULL', _field('init', P0=None)), ('init.H = NULL', _field('init', H=None)),
                        ('method = 9', _set(method=9))] + MODEL_FAULTS + [
    ('cd_ekf on a discrete model', _set(method=F_CD_EKF)),
    ('ekf on an SDE model', _set(model=sde())),
    ('an SDE model without gamma', _both(_set(method=F_CD_EKF, model=sde()), _field('model', gamma=None))),
    ('ekf_for_kpt on the chirp model', _set(method=F_EKF_KPT))] + [
    (f'sgp_filter, {label}', _both(_set(method=F_SGP, sigma=cubature()), edit)) for label, edit in SIGMA_FAULTS]
_SMOOTHER = dict(method=S_EKS, model=lcd(), sigma=None, dt=1e-3, mfs='mfs', Pfs='Pfs', B=1, T=T, mss='mss', Pss='Pss', flags=0)
_KPT_MODEL = Rec(model_id=M_KPT, d=4, n_harm=2, n_params=32, params='lcd', param_stride=0, gamma=None, gamma_stride=0)
_SMOOTHER_ROWS = EMPTY + [('B = -1', _set(B=-1)), ('mfs = NULL', _set(mfs=None)), ('method = 9', _set(method=9)), ('model = NULL', _set(model=None)),
                          ('model.n_params = 4', _field('model', n_params=4)), ('cd_eks on a discrete model', _set(method=S_CD_EKS)),
                          ('sgp_smoother, sigma = NULL', _set(method=S_SGP)), ('the KPT model', _set(model=_KPT_MODEL))]
_SELECT = dict(method=S_EKS, model=lcd(), sigma=None, dt=1e-3, mfs='mfs', Pfs='Pfs', B=1, T=T, out=full_select(), flags=0)
_SMOOTHER_SPLIT = dict(_SMOOTHER, method=S_CD_EKS, model=sde(), segments=2, burn_in=0, junction_err='junction_err')
_CUSTOM_FILTER = dict(m=custom(), sigma=None, params='cparams', param_stride=0, gamma=None, gamma_stride=0, init=init(2), dt=1e-3, ys='ys', ys_stride=T,
                      ys_repeat=1, ys_index=None, B=1, T=T, mfs='mfs2_out', Pfs='Pfs2_out', nll='nll', flags=0)
_CUSTOM_SMOOTHER = dict(m=custom(), sigma=None, params='cparams', param_stride=0, gamma=None, gamma_stride=0, dt=1e-3, mfs='mfs2', Pfs='Pfs2', B=1, T=T,
                        mss='mss2', Pss='Pss2', flags=0)
_CUSTOM_ROWS = EMPTY + [('m = NULL', _set(m=None)), ('B = -1', _set(B=-1)), ('params = NULL', _set(params=None)),
                        ('a sigma-point set with d = 4', _set(sigma=cubature())),
                        ('a model of another device', _field('m', device=1), DERIVED),
                        ('an SDE model without gamma', _field('m', kind=1), DERIVED)]
_POINTS2 = Rec(s=4, d=2, xi='xi', w='w', group_start=None, n_groups=0, flags=0)

ENTRIES = {
    'cgp_filter': dict(good=_FILTER, outputs=('mfs_out', 'Pfs_out', 'nll'), rows=_FILTER_ROWS),
    'cgp_filter_time_split': dict(
        good=dict(_FILTER, segments=2, burn_in=0, junction_err='junction_err'), outputs=('mfs_out', 'Pfs_out', 'nll', 'junction_err'),
        rows=EMPTY + [('segments = 0', _set(segments=0)), ('flags = CGP_SKIP_MISSING', _set(flags=SKIP_MISSING)), ('burn_in = -1', _set(burn_in=-1)),
                      ('junction_err = NULL', _set(junction_err=None)), ('flags = CGP_THREAD_PER_TRIAL', _set(flags=THREAD_PER_TRIAL)),
                      ('kf on a linear model', _set(model=Rec(model_id=M_LINEAR, d=4, n_harm=0, n_params=32, params='lcd', param_stride=0, gamma=None, gamma_stride=0))),
                      ('B = -1', _set(B=-1)), ('ys = NULL', _set(ys=None)), ('model = NULL', _set(model=None)),
                      # the parent zeroed junction_err before it looked at anything else (test_gpu_abi_refusals.py)
                      ('segments = 1, ys = NULL', _set(segments=1, ys=None))]),
    'cgp_smoother': dict(good=_SMOOTHER, outputs=('mss', 'Pss'), rows=_SMOOTHER_ROWS + [('mss = NULL', _set(mss=None))]),
    'cgp_smoother_select': dict(
        good=_SELECT, outputs=('mss', 'Pss', 'comp_mean', 'comp_var', 'expect'),
        rows=EMPTY + [('out = NULL', _set(out=None)), ('mfs = NULL', _set(mfs=None)), ('out.comp = 4', _field('out', comp=4)),
                      ('out.order = 0', _field('out', order=0)), ('out.order = 33', _field('out', order=33)), ('out.func = 4', _field('out', func=4)),
                      ('out.xi = NULL', _field('out', xi=None)), ('model = NULL', _set(model=None)), ('method = 9', _set(method=9)),
                      ('nothing selected, mss = NULL', _field('out', comp_mean=None, comp_var=None, expect=None, mss=None)),
                      ('the generic kernel, mss = NULL', _both(_set(flags=GENERIC_KERNEL), _field('out', mss=None)))]),
    'cgp_smoother_time_split': dict(
        good=_SMOOTHER_SPLIT, outputs=('mss', 'Pss', 'junction_err'),
        rows=EMPTY + [('segments = 0', _set(segments=0)), ('junction_err = NULL', _set(junction_err=None)), ('burn_in = -1', _set(burn_in=-1)),
                      ('flags = CGP_GENERIC_KERNEL', _set(flags=GENERIC_KERNEL)), ('eks on the chirp model', _set(method=S_EKS, model=lcd())),
                      ('mss = NULL', _set(mss=None)), ('model.gamma = NULL', _field('model', gamma=None))]),
    'cgp_smoother_sample': dict(
        good=dict(method=S_EKS, model=lcd(), sigma=None, dt=1e-3, mfs='mfs', Pfs='Pfs', B=1, T=T, S=S, seed=1, trial0=0, sample0=0, normals=None,
                  out=Rec(paths='paths', comp_paths='comp_paths', comp=2, func=0), flags=0),
        outputs=('paths', 'comp_paths'),
        rows=EMPTY + [('S = 0', _set(S=0)), ('S = -1', _set(S=-1)), ('flags = CGP_SKIP_MISSING', _set(flags=SKIP_MISSING)), ('flags = 0x100', _set(flags=0x100)),
                      ('out = NULL', _set(out=None)), ('both outputs NULL', _field('out', paths=None, comp_paths=None)), ('method = 9', _set(method=9)),
                      ('cd_eks', _set(method=S_CD_EKS)), ('model = NULL', _set(model=None)), ('a d = 6 model', _model_d6),
                      ('sgp_smoother, sigma = NULL', _set(method=S_SGP)), ('sgp_smoother, a set of 2000 points', _set(method=S_SGP, sigma=cubature(2000))),
                      ('out.comp = 4', _field('out', comp=4)), ('out.func = 7', _field('out', func=7)), ('trial0 = -1', _set(trial0=-1)),
                      ('mfs = NULL', _set(mfs=None)),
                      ('B = 2^31', _set(B=2 ** 31), DERIVED), ('trial0 + B = 2^32 + 1', _set(trial0=2 ** 32), DERIVED),
                      ('sample0 + S = 2^32 + 1', _set(sample0=2 ** 32 - 1), DERIVED), ('T = 2^31 + 1', _set(T=2 ** 31 + 1), DERIVED)]),
    'cgp_ekf_nll_grad': _tangent('cgp_ekf_nll_grad'),
    'cgp_sgp_nll_grad': _tangent('cgp_sgp_nll_grad'),
    'cgp_ekf_nll_fisher': _tangent('cgp_ekf_nll_fisher'),
    'cgp_sgp_nll_fisher': _tangent('cgp_sgp_nll_fisher'),
    'cgp_cd_ekf_nll_grad': _tangent('cgp_cd_ekf_nll_grad'),
    'cgp_filter_custom': dict(
        good=_CUSTOM_FILTER, outputs=('mfs2_out', 'Pfs2_out', 'nll'),
        rows=_CUSTOM_ROWS + [('ys = NULL', _set(ys=None)), ('ys_repeat = 0', _set(ys_repeat=0)), ('init.m0 = NULL', _field('init', m0=None)),
                             ('a measurement function with a sigma-point set', _both(_set(sigma=_POINTS2), _field('m', kind=2, sgp=0)), DERIVED)]),
    'cgp_smoother_custom': dict(good=_CUSTOM_SMOOTHER, outputs=('mss2', 'Pss2'), rows=_CUSTOM_ROWS + [('mss = NULL', _set(mss=None)), ('a measurement function', _field('m', kind=2, ekf=0, sgp=0), DERIVED)]),
    'cgp_simulate': dict(
        good=dict(model=lcd(), init=init(), dt=1e-3, seed=1, trial0=0, B=1, T=T, xs='xs_out', ys='ys_out', flags=0), outputs=('xs_out', 'ys_out'),
        rows=EMPTY + [('trial0 = -1', _set(trial0=-1)), ('xs = ys = NULL', _set(xs=None, ys=None)), ('model = NULL', _set(model=None)),
                      ('init.m0 = NULL', _field('init', m0=None)), ('init.H = NULL', _field('init', H=None)), ('an SDE model', _set(model=sde())),
                      ('model.d = 6', _field('model', d=6)), ('model.n_params = 4', _field('model', n_params=4)),
                      ('model.param_stride = 1', _field('model', param_stride=1)), ('T = 2^31', _set(T=2 ** 31), DERIVED)]),
    'cgp_simulate_x0': dict(
        good=dict(model=lcd(), init=init(), seed=1, trial0=0, B=1, x0='x0_out'), outputs=('x0_out',),
        rows=[('B = 0', _set(B=0)), ('B = -1', _set(B=-1)), ('model = NULL', _set(model=None)), ('init.P0 = NULL', _field('init', P0=None)),
              ('x0 = NULL', _set(x0=None)), ('model.d = 9', _field('model', d=9))]),
    'cgp_add_noise': dict(
        good=dict(clean='ys', clean_stride=T, Xi='Xi', Xi_stride=0, seed=1, trial0=0, B=1, T=T, ys='ys_out'), outputs=('ys_out',),
        rows=EMPTY + [('trial0 = -1', _set(trial0=-1)), ('clean = NULL', _set(clean=None)), ('clean_stride = 4', _set(clean_stride=4)),
                      ('T = 2^33', _set(T=2 ** 33, clean_stride=0), DERIVED)]),
    'cgp_gaussian_expectation': dict(
        good=dict(ms='ms', sd='sd', n=5, in_stride=1, xi='ghx', w='ghw', order=3, out='expect5'), outputs=('expect5',),
        rows=[('n = 0', _set(n=0)), ('order = 0', _set(order=0)), ('out = NULL', _set(out=None))]),
    'cgp_gaussian_expectation_fn': dict(
        good=dict(func=1, ms='ms', sd='sd', n=5, in_stride=1, xi='ghx', w='ghw', order=3, out='expect5'), outputs=('expect5',),
        rows=[('n = 0', _set(n=0)), ('func = 4', _set(func=4)), ('n = -1', _set(n=-1)), ('order = 0', _set(order=0)), ('xi = NULL', _set(xi=None))]),
    'cgp_squared_error_sums': dict(
        good=dict(a='mfs', r='mss_in', B=1, T=T, d=4, comps=[0, 2], n=2, sums='sums4'), outputs=('sums4',),
        rows=EMPTY + [('n = 9', _set(n=9)), ('d = 0', _set(d=0)), ('comps = NULL', _set(comps=None)), ('comps[1] = 4', _set(comps=[0, 4])),
                      ('B = 65535 x 512 + 1', _set(B=65535 * 512 + 1), DERIVED)]),
    'cgp_pcrlb_sums': dict(
        good=dict(model=lcd(), dt=1e-3, x0='m0', xs='mfs', B=1, T=T, sums='sums26', flags=0), outputs=('sums26',),
        rows=EMPTY + [('B = -1', _set(B=-1)), ('flags = CGP_WAVE_PER_TRIAL', _set(flags=WAVE_PER_TRIAL)), ('model = NULL', _set(model=None)),
                      ('x0 = NULL', _set(x0=None)), ('the La Scala model', _field('model', model_id=M_LASCALA_LCD)),
                      ('an SDE model', _set(model=sde())), ('model.n_params = 4', _field('model', n_params=4)),
                      ('model.param_stride = 5', _field('model', param_stride=5)), ('four harmonics', _field('model', d=10, n_harm=4)),
                      ('B = 65535 x 512 + 1', _set(B=65535 * 512 + 1), DERIVED)]),
    'cgp_debug_math': dict(
        good=dict(op=2, x='x6', n=6, out0='out0', out1='out1'), outputs=('out0', 'out1'),
        rows=[('n = 0', _set(n=0)), ('op = 26', _set(op=26)), ('n = -1', _set(n=-1)), ('op 22 with n = 5', _set(op=22, n=5)), ('x = NULL', _set(x=None))]),
    'cgp_debug_philox': dict(
        good=dict(ctr='ctr', key='key', n=2, out='philox_out'), outputs=('philox_out',),
        rows=[('n = 0', _set(n=0)), ('n = -1', _set(n=-1)), ('key = NULL', _set(key=None))]),
}


def rows(entry):
    """(case id, edit, derived) of every row of an entry point."""
    return [(f'{entry}: {r[0]}', r[1], len(r) > 2 and r[2] == DERIVED) for r in ENTRIES[entry]['rows']]


def arguments(entry, edit=None):
    """A fresh copy of the good call's arguments, edited."""
    a = {k: (Rec(**vars(v)) if isinstance(v, Rec) else list(v) if isinstance(v, list) else v) for k, v in ENTRIES[entry]['good'].items()}
    if edit is not None:
        edit(a)
    return a


# ---- the host program's side -------------------------------------------------------------------------------------------------------------------
def probe_line(entry, a):
    """'<entry> key=value ...': scalars by value (dt left out: nothing checks it), pointers as 0 / 1, a struct's fields as <arg>.<field> behind
    <arg>=0 / 1, the host array comps as comps.n and comps.<i>."""
    words = [entry]
    for k, v in a.items():
        if isinstance(v, Rec):
            words.append(f'{k}=1')
            words += [f'{k}.{f}={x if isinstance(x, int) else int(x is not None)}' for f, x in vars(v).items()]
        elif isinstance(v, list):
            words += [f'{k}=1', f'{k}.n={len(v)}'] + [f'{k}.{i}={x}' for i, x in enumerate(v)]
        elif isinstance(v, float):
            continue
        else:
            words.append(f'{k}={v if isinstance(v, int) else int(v is not None)}')
    return ' '.join(words)


# ---- the device's side -----------------------------------------------------------------------------------------------------------------------------
def buffers():
    """name -> the host array of every buffer the good calls name; the outputs (whatever an entry lists in `outputs`) hold FILL."""
    from chirpgp_amd import filters_smoothers as fs, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    drift, disp, disc, m0, P0, H = pm.build_chirp_model(np.array((0.1, 0.1, 0.1, 1., 1., 7.)))
    rng = np.random.default_rng(7)
    ys = 0.3 * rng.standard_normal(T)
    mfs = m0[None, :] + 0.01 * rng.standard_normal((T, 4))
    cub, gh = SigmaPoints.cubature(4), np.polynomial.hermite_e.hermegauss(3)
    b = dict(lcd=disc.params, sde=fs._drift(drift).params, gamma=fs._gamma_from_callable(disp), H=H, Xi=[0.1], m0=m0, P0=P0, ys=ys,
             mfs=mfs, Pfs=np.tile(P0, (T, 1, 1)), mss_in=mfs + 0.05, xi=cub.xi, w=cub.w, ghx=gh[0], ghw=gh[1] / gh[1].sum(),
             dirs=0.01 * np.cos(np.arange(N_DIR * 27.0)), cparams=[0.9, 0.8, 0.01], H2=[1.0, 0.0], m02=[0.1, 0.2], P02=np.eye(2),
             mfs2=0.1 * rng.standard_normal((T, 2)), Pfs2=np.tile(np.eye(2), (T, 1, 1)), ms=np.linspace(-1, 1, 5), sd=np.linspace(0.5, 1, 5),
             x6=np.linspace(0.1, 2, 6))
    b = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in b.items()}
    b.update(ctr=np.arange(8, dtype=np.uint32), key=np.array([3, 4], dtype=np.uint32), philox_out=np.full(8, 0xABABABAB, dtype=np.uint32))
    shapes = dict(mfs_out=(T, 4), Pfs_out=(T, 16), nll=(T,), junction_err=(1,), mss=(T, 4), Pss=(T, 16), comp_mean=(T,), comp_var=(T,), expect=(T,),
                  paths=(S, T, 4), comp_paths=(S, T), nll1=(1,), grad=(N_DIR,), fisher=(N_DIR, N_DIR), mfs2_out=(T, 2), Pfs2_out=(T, 4), mss2=(T, 2),
                  Pss2=(T, 4), xs_out=(T, 4), ys_out=(T,), x0_out=(4,), expect5=(5,), sums4=(4, T), sums26=(26, T), out0=(6,), out1=(6,))
    b.update({k: np.full(s, FILL) for k, s in shapes.items()})
    return b


_SCALARS = {'method': C.c_int, 'func': C.c_int, 'op': C.c_int, 'dt': C.c_double, 'flags': C.c_uint32, 'seed': C.c_uint64, 'n_dir': C.c_int32,
            'order': C.c_int32, 'd': C.c_int32}      # every other scalar is an int64_t; `n` is int32_t in cgp_squared_error_sums alone


def call(lib, ctx, entry, a, address, custom_model=None):
    """The entry point of the loaded library `lib` with the arguments `a`; address(name) is the device address of a buffer.
    -> (return code, cgp_last_error's message, '' where the code is 0)."""
    from chirpgp_amd import _engine as E
    structs = {'model': E.CgpModel, 'sigma': E.CgpSigma, 'init': E.CgpInit}
    keep, args = [], [ctx]
    for k, v in a.items():
        if k == 'm':
            args.append(custom_model if v is not None else None)
        elif isinstance(v, Rec):
            cls = structs.get(k) or (E.CgpSampleOut if entry == 'cgp_smoother_sample' else E.CgpSmoothOut)
            s = cls(**{f: (x if isinstance(x, int) else address(x) if x is not None else None) for f, x in vars(v).items()})
            keep.append(s)
            args.append(C.byref(s))
        elif isinstance(v, list):
            keep.append((C.c_int32 * len(v))(*v))
            args.append(keep[-1])
        elif isinstance(v, str) or v is None:
            args.append(C.c_void_p(address(v)) if v is not None else None)
        elif k == 'n' and entry == 'cgp_squared_error_sums':
            args.append(C.c_int32(v))
        else:
            args.append(_SCALARS.get(k, C.c_int64)(v))
    fn = getattr(lib, entry)
    fn.restype = C.c_int
    rc = fn(*args, None)                               # (the null stream)
    lib.cgp_last_error.restype = C.c_char_p
    return rc, (lib.cgp_last_error(ctx).decode() if rc else '')


class Device:
    """The buffers of buffers() on the GPU and CUSTOM_BODY compiled by `lib` (a loaded libchirpgp_hip.so, with its context `ctx`; the
    headers under include_dir must be that library's): run() is one call of the table with the entry's outputs pre-filled."""

    def __init__(self, lib, ctx, include_dir):
        import torch
        self.torch, self.lib, self.ctx = torch, lib, ctx
        self.host = buffers()
        self.dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in self.host.items()}
        self.custom = C.c_void_p()
        lib.cgp_last_error.restype = C.c_char_p
        rc = lib.cgp_model_from_source(ctx, C.c_int(CUSTOM_KIND), C.c_int32(CUSTOM_D), CUSTOM_BODY.encode(), include_dir.encode(), C.byref(self.custom))
        assert rc == 0, lib.cgp_last_error(ctx)

    def close(self):
        self.lib.cgp_custom_model_destroy.restype = None
        self.lib.cgp_custom_model_destroy(self.custom)

    def run(self, entry, edit=None):
        """-> (return code, message, {output name: its content after the call}); before the call every output of the entry holds its pre-fill."""
        outputs = ENTRIES[entry]['outputs']
        for name in outputs:
            self.dev[name].copy_(self.torch.from_numpy(self.host[name].view(np.int32) if self.host[name].dtype == np.uint32 else self.host[name]))
        self.torch.cuda.synchronize()
        rc, msg = call(self.lib, self.ctx, entry, arguments(entry, edit), lambda name: self.dev[name].data_ptr(), self.custom)
        self.torch.cuda.synchronize()
        return rc, msg, {name: self.dev[name].cpu().numpy().view(self.host[name].dtype) for name in outputs}

    def untouched(self, name, after):
        return np.array_equal(after.view(np.uint8), self.host[name].view(np.uint8))
