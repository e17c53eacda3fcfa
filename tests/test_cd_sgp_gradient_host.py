"""The host half of cgp_sgp_nll_grad on the SDE model (the continuous-discrete sigma-point filter's tangent kernel,
csrc/cgp_tangent4_cd_sigma.hpp), without a GPU: the float64 NumPy restatement of the recursion with its forward tangents
(tests/cd_sgp_grad_oracle.py) against every case of the 100-digit fixture tests/golden/exact_cd_sgp_grad.npz, a decade inside the gates the
kernel is held to (tests/test_gpu_cd_sgp_gradient.py) -- float64 reaches them before the GPU is asked to; the fixture holds what it must;
mle.has_tangent_kernel admits exactly what is built while mle.has_exact_gradient keeps its answers; the engine binding asks for 27 doubles
a direction with gamma and 24 without; no symbol was added and the version stands; and what prepare_tangent (csrc/cgp_args.hpp) makes of
an SDE model, asked through the host program tests/abi_probe.hip.

RESULTS (printed by the tests, none of them set a gate): the restatement's worst value error over the fixture 3.3e-15 (random_cds_01),
worst gradient error 7.7e-15 of its scale (random_cds_04); over the record lengths of the GPU test <= 5.5e-16 / 2.1e-15.  Every admitted
case is three decades and more inside 1e-11 / 1e-8: none had to be dropped or narrowed for the oracle's sake.  The draws: 21 drawn, 5
rejected (the 100-digit run itself lost a Cholesky factor inside an RK4 step), 16 kept."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import abi_cases as ac
from tests import cd_sgp_grad_oracle as so
from tests.cd_sgp_grad_cases import (GRAD_GATE, GRAD_MOVE_MAX, NAMES, PREFIX_NAMES, PREFIX_T, VALUE_MOVE_MAX, VALUE_RTOL, Z, case, errors,
                                     gates)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECADE = 10.0
SKIP_MISSING = 0x2000                                  # include/chirpgp_hip.h: CGP_SKIP_MISSING


# ------------------------------------------------------------------------------------------------ 1. the fixture and the oracle
def test_the_fixture_holds_what_it_must():
    cs = [case(n) for n in NAMES]
    groups = {c['group'] for c in cs}
    assert groups == {'prefix', 'random_cds', 'edge', 'other', 'gaps', 'substeps'}
    assert {c['sigma'] for c in cs if c['group'] == 'prefix'} == {'cubature', 'gh3'}
    for n in PREFIX_NAMES:
        assert Z[f'{n}.nll_prefix'].shape == (130,) and Z[f'{n}.grad_prefix'].shape == (130, 6)
    rnd = [c for c in cs if c['group'] == 'random_cds']
    drawn, rejected = int(Z['drawn.random_cds']), int(Z['rejected.random_cds'])
    print(f'random_cds: {drawn} drawn, {rejected} rejected, {len(rnd)} kept')
    assert len(rnd) >= 12 and 4 * len(rnd) >= 3 * drawn and drawn - rejected == len(rnd)
    assert {c['build'] for c in rnd} == {'chirp', 'lascala'} and {c['dt'] for c in rnd} == {1e-3, 1e-2} and {c['lost'] for c in rnd} == {0, 1}
    assert {c['sigma'] for c in cs} == {'cubature', 'gh3', 'gh4'}
    assert sum(c['skip'] for c in cs) == 6 and {c['n'] for c in cs if c['group'] == 'substeps'} == {2, 4}
    assert case('edge_cds_lam0')['theta'][0] == -800. and case('other_cds_H_dXi')['with_dxi'] == 1 and case('other_cds_H_dXi')['grad'].size == 7
    for c in cs:
        if c['group'] != 'edge':
            assert c['moved_nll'] < VALUE_MOVE_MAX and c['moved_grad'] < GRAD_MOVE_MAX, c['name']
    e = case('gaps_cds_everywhere')
    assert e['nll'] == 0.0 and not e['grad'].any() and np.isnan(e['ys']).all()


def _oracle(c, T=None):
    ys = c['ys'] if T is None else c['ys'][:T]
    return so.value_and_grad(c['build'], c['sigma'], c['theta'], ys, c['Xi'], c['dt'], H=c['H'], with_dxi=bool(c['with_dxi']),
                             skip_missing=bool(c['skip']), substeps=c['n'])


def test_float64_oracle_is_a_decade_inside_the_gates_on_every_case():
    """The GPU gates (value 1e-11 relative, gradient 1e-8 of its scale) are usable only if float64 itself stays a decade inside them."""
    worst = [0., '', 0., '']
    for name in NAMES:
        c = case(name)
        f, g_ = _oracle(c)
        ev, eg = errors(f[-1], g_[-1], c['nll'], c['grad'], name)
        vg, gg = gates(c)
        assert ev < vg / DECADE and eg < gg / DECADE, name
        if ev > worst[0]:
            worst[:2] = [ev, name]
        if eg > worst[2]:
            worst[2:] = [eg, name]
    print(f'worst value error {worst[0]:.2e} ({worst[1]}), worst gradient error {worst[2]:.2e} ({worst[3]})')


@pytest.mark.parametrize('name', PREFIX_NAMES)
def test_float64_oracle_on_the_record_lengths(name):
    c = case(name)
    f, g_ = _oracle(c)
    worst = [0., 0.]
    for T in PREFIX_T:
        ev, eg = errors(f[T - 1], g_[T - 1], Z[f'{name}.nll_prefix'][T - 1], Z[f'{name}.grad_prefix'][T - 1], f'{name} T = {T}')
        worst = [max(worst[0], ev), max(worst[1], eg)]
        assert ev < VALUE_RTOL / DECADE and eg < GRAD_GATE / DECADE, T
    print(f'{name}: worst over the record lengths: value {worst[0]:.2e}, gradient {worst[1]:.2e}')


def test_substeps_are_steps_of_the_refined_record():
    """n substeps = the gapped filter on the n-times refined record (NaN between the samples) at dt / n: the oracle's two routes agree."""
    c = case('substeps_cds_n2')
    fine = np.full(c['ys'].size * 2, np.nan)
    fine[1::2] = c['ys']
    f, g_ = _oracle(c)
    f2, g2 = so.value_and_grad(c['build'], c['sigma'], c['theta'], fine, c['Xi'], c['dt'] / 2, skip_missing=True)
    assert abs(f[-1] - f2[-1]) <= 1e-13 * abs(f[-1]) and np.abs(g_[-1] - g2[-1]).max() <= 1e-12 * np.abs(g_[-1]).max()


# ------------------------------------------------------------------------------------------------ 2. the predicates
def test_has_tangent_kernel_admits_what_is_built_and_has_exact_gradient_is_unchanged():
    from chirpgp_amd import mle, models as pm
    from chirpgp_amd.quadratures import SigmaPoints
    gh3, gh3_d6 = SigmaPoints.gauss_hermite(4, 3), SigmaPoints.cubature(6)
    assert 'has_tangent_kernel' in mle.__all__
    for build in (pm.build_chirp_model, pm.build_lascala_model):
        assert mle.has_tangent_kernel('cd_sgp_filter', build, 0.1, sgps=gh3)
        assert mle.has_tangent_kernel('cd_sgp_filter', build, 0.1, sgps=SigmaPoints.cubature(4))
        assert not mle.has_tangent_kernel('cd_sgp_filter', build, 0.1)                              # no set
        assert not mle.has_tangent_kernel('cd_sgp_filter', build, 0.1, sgps=gh3_d6)
        assert not mle.has_tangent_kernel('cd_sgp_filter', build, np.array([0.1, 0.2]), sgps=gh3)  # a per-trial Xi: the difference form
        assert not mle.has_exact_gradient('cd_sgp_filter', build, 0.1, sgps=gh3)                    # the older predicate keeps its answer
    assert not mle.has_tangent_kernel('cd_sgp_filter', pm.build_harmonic_chirp_model, 0.1, sgps=gh3)
    assert not mle.has_tangent_kernel('cd_sgp_smoother', pm.build_chirp_model, 0.1, sgps=gh3)
    assert not mle.has_tangent_kernel('cd_eks', pm.build_chirp_model, 0.1)
    # true wherever has_exact_gradient is, and nowhere else but for 'cd_sgp_filter'
    for method in ('ekf', 'cd_ekf', 'sgp_filter', 'eks', 'ekf_for_kpt'):
        for build in (pm.build_chirp_model, pm.build_lascala_model, pm.build_harmonic_chirp_model):
            for Xi in (0.1, np.array([0.1, 0.2])):
                for sg in (None, gh3, gh3_d6):
                    assert mle.has_tangent_kernel(method, build, Xi, sg) == mle.has_exact_gradient(method, build, Xi, sg), (method, build, sg)
    assert not mle._exact_by_default('cd_sgp_filter', pm.build_chirp_model, 0.1, 10 ** 6, {})      # no default moves
    assert not mle._has_fisher_form('cd_sgp_filter')
    assert re.search('exact=True', str(mle._exact_unsupported())) and re.search('tangent kernel', str(mle._exact_unsupported()))
    assert 'three' in mle.has_exact_gradient.__doc__.lower() or 'older' in mle.has_exact_gradient.__doc__.lower()


def test_the_front_ends_refuse_before_anything_is_built():
    from chirpgp_amd import mle, models as pm
    from chirpgp_amd.quadratures import SigmaPoints

    def build(*a, **k):
        raise AssertionError('the builder was called')
    gh3 = SigmaPoints.gauss_hermite(4, 3)
    th, ys = np.zeros((1, 6)), np.zeros(8)
    with pytest.raises(ValueError, match='exact=True'):       # an unknown builder has no directions
        mle.value_and_grad(build, th, ys, 0.1, 1e-3, method='cd_sgp_filter', sgps=gh3)
    with pytest.raises(ValueError, match='exact=True'):       # no sigma-point set
        mle.make_objective('cd_sgp_filter', pm.build_chirp_model, ys, 0.1, 1e-3, exact=True)
    with pytest.raises(ValueError, match='1 .. 16'):
        mle.value_and_grad(pm.build_chirp_model, th, ys, 0.1, 1e-3, method='cd_sgp_filter', sgps=gh3, substeps=17)
    for call in (lambda: mle.value_grad_fisher(pm.build_chirp_model, th, ys, 0.1, 1e-3, method='cd_sgp_filter', sgps=gh3),
                 lambda: mle.standard_errors(pm.build_chirp_model, th[0], ys, 0.1, 1e-3, method='cd_sgp_filter', sgps=gh3),
                 lambda: mle.fit_scoring('cd_sgp_filter', pm.build_chirp_model, [1.] * 6, ys, 0.1, 1e-3, sgps=gh3)):
        with pytest.raises(ValueError, match="'cd_sgp_filter'.*Fisher form"):
            call()


# ------------------------------------------------------------------------------------------------ 3. the binding and the ABI
def test_the_binding_takes_27_doubles_with_gamma_and_24_without(monkeypatch):
    """_run_nll_grad checks the directions' shape before it touches the device: stand-ins for what comes before."""
    from chirpgp_amd import _engine as E

    class Rec1:
        ndim, shape = 2, (1, 8)
    monkeypatch.setattr(E, '_torch', lambda: None)
    monkeypatch.setattr(E, 'dev', lambda x, *a: Rec1())
    monkeypatch.setattr(E, '_check_dimension', lambda spec: 4)
    args = (None, np.eye(4), 'a set', None, 0.1, None, None, 1e-3, None)
    with pytest.raises(ValueError, match=r'dirs must be \(1, n_dir, 27\)'):
        E.run_cd_sgp_nll_grad(*args, np.zeros((1, 6, 24)))
    with pytest.raises(ValueError, match=r'dirs must be \(1, n_dir, 24\)'):
        E.run_sgp_nll_grad(None, 'a set', None, 0.1, None, None, 1e-3, None, np.zeros((1, 6, 27)))
    with pytest.raises(ValueError, match='gamma'):
        E.run_cd_sgp_nll_grad(None, None, 'a set', None, 0.1, None, None, 1e-3, None, np.zeros((1, 6, 27)))
    with pytest.raises(ValueError, match='sigma-point set'):
        E.run_cd_sgp_nll_grad(None, np.eye(4), None, None, 0.1, None, None, 1e-3, None, np.zeros((1, 6, 27)))
    assert E.CD_DIR_DOUBLES == 27 and E.DIR_DOUBLES == 24


def test_no_symbol_was_added_and_the_version_stands():
    import __graft_entry__ as ge
    ge.build()
    from chirpgp_amd import _engine as E
    from tests.test_abi import HEADER
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r'\bint\s+(cgp_\w+)\s*\(', src)) | set(re.findall(r'\b(?:const char\s*\*|void|cgp_ctx\s*\*)\s*(cgp_\w+)\s*\(', src))
    assert not [n for n in declared | set(E.EXPORTS) if 'cd_sgp' in n]
    assert 'cgp_sgp_nll_grad' in E.EXPORTS and 'cgp_cd_ekf_nll_grad' in E.EXPORTS
    assert len(re.findall(r'#define\s+CGP_\w*DIR_DOUBLES\b', src)) == 2               # CGP_DIR_DOUBLES, CGP_CD_DIR_DOUBLES: no third
    assert E.load_library().cgp_version() == 160
    text = open(HEADER).read()
    comment = text[text.index('/* The same for the sigma-point filter'):text.index('int cgp_sgp_nll_grad(')]      # the entry's own comment
    assert 'CGP_M_HARMONIC_SDE' in comment and 'CGP_CD_DIR_DOUBLES' in comment and 'CGP_RK4_SUBSTEPS' in comment


# ------------------------------------------------------------------------------------------------ 4. prepare_tangent on an SDE model
@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    """lines -> the answers of tests/abi_probe.hip (built as tests/test_abi_refusals.py builds it: host code only)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path_factory.mktemp('abi_probe_cds') / 'abi_probe')
    subprocess.run([hipcc, '--cuda-host-only', '-no-hip-rt', '-O1', '-std=c++17', '-Wno-int-to-pointer-cast', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'abi_probe.hip'), '-o', exe], check=True)

    def ask(entry, *edits):
        a = ac.arguments(entry, ac._both(*edits))
        return subprocess.run([exe], input=ac.probe_line(entry, a) + '\n', capture_output=True, text=True, check=True).stdout.strip()
    return ask


def test_prepare_tangent_on_an_sde_model(probe):
    from chirpgp_amd import _engine as E
    sde = ac._set(model=ac.sde())
    n4 = E.rk4_substeps(4)
    assert n4 and not n4 & SKIP_MISSING
    grad, fisher = 'cgp_sgp_nll_grad', 'cgp_sgp_nll_fisher'
    assert probe(grad, sde) == 'ok'
    assert probe(grad, sde, ac._set(flags=SKIP_MISSING)) == 'ok'
    assert probe(grad, sde, ac._set(flags=n4)) == 'ok'
    assert probe(grad, sde, ac._set(flags=n4 | SKIP_MISSING)) == 'ok'
    assert probe(grad, sde, ac._field('sigma', s=1000)) == 'ok'
    # ---- the Fisher entry refuses it, in its own words
    got = probe(fisher, sde)
    assert got.startswith(f'refused {ac.E_UNSUPPORTED}: ') and fisher in got and 'Fisher form of the continuous-discrete filters is not built' in got, got
    # ---- another shape, no gamma: the message names the accepted shape
    for edit in (ac._field('model', gamma=None), ac._field('model', d=6, n_harm=2), ac._field('model', n_params=5)):
        got = probe(grad, sde, edit)
        assert got.startswith(f'refused {ac.E_UNSUPPORTED}: ') and grad in got, got
        assert all(w in got for w in ('CGP_M_HARMONIC_SDE', 'n_harm = 1', 'd = 4', 'n_params = 3', 'model.gamma')), got
    assert probe(grad, sde, ac._field('model', gamma_stride=1)) == f'refused {ac.E_ARG}: model.gamma_stride < d * d'
    # ---- the checks behind the model keep their order and words
    assert probe(grad, sde, ac._field('model', param_stride=1)) == f'refused {ac.E_ARG}: model.param_stride < n_params'
    assert probe(grad, sde, ac._set(flags=n4 | 0x2)) == f'refused {ac.E_ARG}: {grad} takes CGP_SKIP_MISSING and no other flag: bit 0x2 (CGP_WAVE_PER_TRIAL) is set'
    assert probe(grad, sde, ac._set(B=2 ** 31)) == f'refused {ac.E_UNSUPPORTED}: {grad} runs one workgroup per trial: B must be < 2^31'
    # (the parked RK4 state shares LDS with the staged set: 1100 points fit the discrete form's stage and not this one's)
    assert probe(grad, ac._field('sigma', s=1100)) == 'ok'
    assert probe(grad, sde, ac._field('sigma', s=1100)) == f'refused {ac.E_UNSUPPORTED}: the sigma-point set does not fit the LDS stage of {grad}'
    # ---- substeps bits with an LCD model: today's flag message, on both entry points
    lowest = n4 & -n4
    for entry in (grad, fisher):
        assert probe(entry, ac._set(flags=n4)) == (f'refused {ac.E_ARG}: {entry} takes CGP_SKIP_MISSING and no other flag: bit 0x{lowest:x} '
                                                   '(CGP_RK4_SUBSTEPS) is set')
