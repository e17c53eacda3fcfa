"""The exact gradient and the Fisher information on records with gaps: cgp_ekf_nll_grad, cgp_sgp_nll_grad, cgp_ekf_nll_fisher and
cgp_sgp_nll_fisher with CGP_SKIP_MISSING (csrc/cgp_tangent4.hpp, cgp_tangent4_sigma.hpp: the GAPS instantiations) against 100-digit
arithmetic (tests/golden/exact_gaps_grad.npz, tests/golden/make_exact_gaps_grad.py), the identities a skipped step must satisfy bit for
bit, the flag's boundaries, and the layer on top in chirpgp_amd/mle.py (missing='skip' in value_and_grad, value_grad_fisher,
standard_errors, fit_scoring).

Gates: the unflagged tests' own (test_gpu_gradient_edges.py, test_gpu_fisher.py) -- value 1e-11 relative, gradient 1e-8 of its largest
component, Fisher 1e-8 of its largest entry, Fisher exactly symmetric.

Measured on MI355X (gfx950), every case of the fixture:
  * cgp_ekf_nll_grad and cgp_ekf_nll_fisher, 19 cases: value <= 1.45e-12 (random_ekf_21__mixed), gradient <= 9.11e-12 of its scale
    (random_ekf_09__mixed, whose own movement under the admission rule is 2.0e-13), fisher <= 2.91e-12 (random_ekf_21__mixed);
  * cgp_sgp_nll_grad and cgp_sgp_nll_fisher, 7 cases: value <= 5.23e-13, gradient <= 2.45e-11, fisher <= 7.11e-11 (all random_gh3_08__mixed);
  * the fourteen patterns in one launch: every row bit-equal to the record launched alone, both EKF entry points;
  * the flag on a record without NaN: the unflagged call's bits in all four entry points (asserted at 1e-11 of scale).

On the parent commit every test here fails: `missing` is an unknown keyword, the flags word is ignored and a NaN propagates."""
import os
import subprocess
import sys

import numpy as np
import numpy.testing as npt
import pytest

from tests import gap_oracle as go
from tests.gaps_grad_cases import NAMES, SKIP_MISSING, gaps_case, raw, run
from tests.golden import make_exact_gaps_grad as gen
from tests.tangent_cases import ENTRIES, grad_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_RTOL, GRAD_GATE, FISHER_GATE = 1e-11, 1e-8, 1e-8
PREFIX_EKF = [gen.case_name('prefix_ekf', p) for p in gen.PATTERNS]
_results = {}


def _errors(c, f, g, F=None):
    ev = abs(f - c['nll']) / abs(c['nll'])
    eg = float(np.abs(g - c['grad']).max() / np.abs(c['grad']).max())
    eF = None if F is None else float(np.abs(F - c['fisher']).max() / np.abs(c['fisher']).max())
    return ev, eg, eF


def _fixture_result(name):
    """A fixture case through its method's gradient and Fisher entry points, flagged, computed once:
    -> (case, (nll, grad) of *_nll_grad, (nll, grad, F) of *_nll_fisher, their errors)."""
    if name not in _results:
        c = gaps_case(name)
        a, b = run(c, False), run(c, True)
        _results[name] = (c, a, b, _errors(c, a[0][0], a[1][0]), _errors(c, b[0][0], b[1][0], b[2][0]))
    return _results[name]


def _entry(c, fisher):
    return f'cgp_{"ekf" if c["method"] == "ekf" else "sgp"}_nll_{"fisher" if fisher else "grad"}'


# ------------------------------------------------------------------------------------------------ 1. every fixture case
@pytest.mark.parametrize('name', NAMES)
def test_fixture_case(name):
    """Value, gradient and Fisher matrix of the observed samples within the unflagged tests' gates of 100-digit arithmetic, from the
    gradient entry point and from the Fisher entry point of the case's method; F exactly symmetric."""
    c, a, b, ea, eb = _fixture_result(name)
    print(f'{name} ({c["n_observed"]} of {c["ys"].size} observed): {_entry(c, False)} value {ea[0]:.2e}, gradient {ea[1]:.2e}; '
          f'{_entry(c, True)} value {eb[0]:.2e}, gradient {eb[1]:.2e}, fisher {eb[2]:.2e} of its scale {np.abs(c["fisher"]).max():.3g}')
    assert b[2].shape == (1,) + c['fisher'].shape and a[1].shape == (1, c['n_dir'])
    npt.assert_array_equal(b[2], b[2].transpose(0, 2, 1))
    assert ea[0] < VALUE_RTOL and eb[0] < VALUE_RTOL, (a[0], b[0], c['nll'])
    assert ea[1] < GRAD_GATE and eb[1] < GRAD_GATE, (a[1], b[1], c['grad'])
    assert eb[2] < FISHER_GATE, (b[2][0], c['fisher'])


def test_no_fixture_case_is_left_out_and_the_worst_per_entry_point():
    """All 26 cases of the generator's list are in the file and run above; the worst errors per entry point, for docs/KERNELS.md."""
    assert sorted(NAMES) == sorted(gen.case_name(s, p) for line in gen.CASES for s, p in line)
    for method in ('ekf', 'sgp_filter'):
        rows = [r for r in map(_fixture_result, NAMES) if r[0]['method'] == method]
        assert rows
        for fisher, k in ((False, 3), (True, 4)):
            labels = ('value', 'gradient') + (('fisher',) if fisher else ())
            worst = [max(rows, key=lambda r: r[k][i]) for i in range(len(labels))]
            print(f'{_entry(rows[0][0], fisher)}, {len(rows)} cases: ' + ', '.join(f'worst {label} error {r[k][i]:.2e} ({r[0]["name"]})'
                                                                               for i, (label, r) in enumerate(zip(labels, worst))))


# ------------------------------------------------------------------------------------------------ 2. fourteen records, fourteen gap patterns, one launch
@pytest.mark.parametrize('fisher', [False, True], ids=['cgp_ekf_nll_grad', 'cgp_ekf_nll_fisher'])
def test_fourteen_patterns_in_one_launch(fisher):
    """The 14 prefix_ekf patterns as B = 14 records with their own gaps, six directions: 84 lanes, so that trial 10 straddles two wavefronts
    of the gradient kernel, and two blocks of 10 whole trials in the Fisher kernel -- the gate is per lane.  Every row within the gates of
    exact arithmetic, and (measured on the MI355X, and asserted) bit-equal to the same record launched alone, B = 1."""
    cases = [gaps_case(n) for n in PREFIX_EKF]
    ys = np.stack([c['ys'] for c in cases])
    assert ys.shape == (14, 130)
    got = run(cases[0], fisher, ys=ys)
    alone = [run(c, fisher) for c in cases]
    equal = True
    for b, c in enumerate(cases):
        ev, eg, eF = _errors(c, got[0][b], got[1][b], got[2][b] if fisher else None)
        same = all(np.array_equal(got[k][b], alone[b][k][0]) for k in range(len(got)))
        equal &= same
        print(f'{c["name"]}: row {b} value {ev:.2e}, gradient {eg:.2e}' + (f', fisher {eF:.2e}' if fisher else '') + f', bit-equal to B = 1: {same}')
        assert ev < VALUE_RTOL and eg < GRAD_GATE and (eF is None or eF < FISHER_GATE), (c['name'], ev, eg, eF)
        if fisher:
            npt.assert_array_equal(got[2][b], got[2][b].T)
    assert equal


# ------------------------------------------------------------------------------------------------ 3. identities, bit for bit
def _id_case(entry):
    return grad_case('prefix_ekf' if '_ekf_' in entry else 'prefix_gh3')


def _run_entry(entry, c, ys, missing='skip'):
    return run(c, entry.endswith('_fisher'), ys=ys, missing=missing)


@pytest.mark.parametrize('entry', ENTRIES)
def test_trailing_gaps_add_nothing(entry):
    """n observed samples followed by k NaN: every output equals the flagged run on the n samples alone, bit for bit -- across the EKF
    kernel's 8-step block (7 + 1, 8 + 1, 9 + 7), the sigma-point kernel's 64-step chunk (64 + 1, 65 + 65) and for one sample with 129."""
    c = _id_case(entry)
    for n, k in ((7, 1), (8, 1), (9, 7), (64, 1), (65, 65), (1, 129)):
        ys = c['ys'][:n]
        want = _run_entry(entry, c, ys)
        got = _run_entry(entry, c, np.concatenate([ys, np.full(k, np.nan)]))
        assert all(np.isfinite(w).all() for w in want) and np.abs(want[1]).max() > 0
        for w, g, what in zip(want, got, ('nll', 'grad', 'fisher')):
            npt.assert_array_equal(g, w, err_msg=f'{entry}: {what}, {n} samples + {k} NaN')


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_record_of_nan_only_and_an_empty_record(entry):
    """T = 1, 9, 130, every sample missing: nll = +0.0, grad = 0 and fisher = 0 -- the likelihood of no samples.  T = 0 with the flag still
    writes zeros.  (The C entry point itself, buffers pre-filled.)"""
    c = _id_case(entry)
    for T in (1, 9, 130):
        rc, msg, nll, grad, F = raw(entry, c, np.full((2, T), np.nan), SKIP_MISSING)
        assert rc == 0, msg
        npt.assert_array_equal(nll, 0.0)
        assert not np.signbit(nll).any()
        npt.assert_array_equal(grad, 0.0)
        if entry.endswith('_fisher'):
            npt.assert_array_equal(F, 0.0)
    rc, msg, nll, grad, F = raw(entry, c, np.full((2, 1), np.nan), SKIP_MISSING, T=0)
    assert rc == 0, msg
    npt.assert_array_equal(nll, 0.0); npt.assert_array_equal(grad, 0.0)
    if entry.endswith('_fisher'):
        npt.assert_array_equal(F, 0.0)


# ------------------------------------------------------------------------------------------------ 4. the flag's boundaries
@pytest.mark.parametrize('entry', ENTRIES)
def test_flag_changes_nothing_on_a_record_without_gaps(entry):
    """Flagged against unflagged on the T = 130 record: within 1e-11 of scale, the tolerance test_gpu_fisher.py gives two compilations of
    the same step (the GAPS kernels are units of their own)."""
    c = _id_case(entry)
    want, got = _run_entry(entry, c, c['ys'], missing=None), _run_entry(entry, c, c['ys'])
    for w, g, what in zip(want, got, ('nll', 'grad', 'fisher')):
        print(f'{entry}: {what} differs by {np.abs(g - w).max() / np.abs(w).max():.2e} of its scale')
        npt.assert_allclose(g, w, rtol=0, atol=1e-11 * np.abs(w).max(), err_msg=what)


@pytest.mark.parametrize('entry', ENTRIES)
def test_without_the_flag_a_gap_is_still_poison(entry):
    """Unflagged (missing=None and 'propagate') on the `mixed` record: NaN in every output, as before."""
    c = _id_case(entry)
    ys = go.with_gaps(c['ys'], gen.mixed(130))
    for missing in (None, 'propagate'):
        for o in _run_entry(entry, c, ys, missing=missing):
            assert np.isnan(o).all(), (entry, missing, o)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('value', [np.inf, -np.inf])
def test_inf_is_a_measurement_not_a_gap(entry, value):
    """+-inf at step 40 of the T = 130 record, flagged: not skipped -- the outputs are the unflagged call's on that record (an infinite
    innovation leaves nothing finite; NaN compares equal to NaN), and they stay so with real gaps beside it."""
    c = _id_case(entry)
    ys = np.array(c['ys'])
    ys[40] = value
    want = _run_entry(entry, c, ys, missing=None)
    got = _run_entry(entry, c, ys)
    for w, g, what in zip(want, got, ('nll', 'grad', 'fisher')):
        assert not np.isfinite(g).any(), (entry, what, g)
        npt.assert_array_equal(g, w, err_msg=what)                       # (NaN equals NaN here)
    gapped = go.with_gaps(ys, ((0, 1), (6, 10), (60, 70)))               # and beside real gaps: still not skipped
    for g in _run_entry(entry, c, gapped):
        assert not np.isfinite(g).any(), (entry, g)


@pytest.mark.parametrize('entry', ENTRIES)
def test_any_other_flag_bit_is_refused_by_name(entry):
    """CGP_E_ARG with the bit's name, alone and beside CGP_SKIP_MISSING, and nothing written."""
    c = _id_case(entry)
    ys = c['ys'][None, :16]
    for flags, name in ((0x1, b'CGP_NLL_FINAL_ONLY'), (SKIP_MISSING | 0x4, b'CGP_THREAD_PER_TRIAL'), (SKIP_MISSING | 0x800, b'CGP_TIME_SPLIT'),
                        (0x4000, b'0x4000')):
        rc, msg, nll, grad, F = raw(entry, c, ys, flags)
        assert rc == -1 and name in msg and entry.encode() in msg, (flags, rc, msg)
        npt.assert_array_equal(nll, 123.0); npt.assert_array_equal(grad, 123.0); npt.assert_array_equal(F, 123.0)


@pytest.mark.parametrize('entry', ENTRIES)
def test_every_output_is_written(entry):
    """Three records (no gap, `mixed`, all but step 65), buffers pre-filled: every entry of nll, grad and (the Fisher forms) fisher is
    overwritten with a finite number, and the rows are the engine's."""
    c = _id_case(entry)
    ys = np.stack([c['ys'], go.with_gaps(c['ys'], gen.mixed(130)), go.with_gaps(c['ys'], gen.all_but(130, 65))])
    rc, msg, nll, grad, F = raw(entry, c, ys, SKIP_MISSING, fill=123.0)
    assert rc == 0, msg
    outs = (nll, grad) + ((F,) if entry.endswith('_fisher') else ())
    for o, w in zip(outs, _run_entry(entry, c, ys)):
        assert np.isfinite(o).all() and not (o == 123.0).any()
        npt.assert_array_equal(o, w)
    if not entry.endswith('_fisher'):
        npt.assert_array_equal(F, 123.0)                                 # (not handed over: untouched)


# ------------------------------------------------------------------------------------------------ 5. chirpgp_amd.mle
def test_mle_value_and_grad_on_shared_gapped_records():
    """Two records with different gaps shared over four parameter rows through record_index: value_and_grad(missing='skip') gives
    batched_nll(missing='skip')'s value at 1e-9 (two kernels, the gaps tests' gate) and a finite gradient; value_grad_fisher the same
    value and gradient as value_and_grad at 1e-11 of scale."""
    from chirpgp_amd import mle, models as pm
    c = grad_case('prefix_ekf')
    recs = np.stack([go.with_gaps(c['ys'], gen.mixed(130)), go.with_gaps(c['ys'], gen.odd(130))])
    rng = np.random.default_rng(8)
    thetas = c['theta'][None, :] + 0.05 * rng.standard_normal((4, 6))
    idx = np.array([0, 1, 1, 0])
    want = mle.batched_nll('ekf', pm.build_chirp_model, thetas, recs, c['Xi'], c['dt'], record_index=idx, missing='skip')
    f, g = mle.value_and_grad(pm.build_chirp_model, thetas, recs, c['Xi'], c['dt'], record_index=idx, missing='skip')
    print('value_and_grad against batched_nll:', np.abs(f - want) / np.abs(want))
    assert np.isfinite(want).all() and f.shape == (4,) and g.shape == (4, 6) and np.isfinite(g).all()
    npt.assert_allclose(f, want, rtol=1e-9)
    f2, g2, F2 = mle.value_grad_fisher(pm.build_chirp_model, thetas, recs, c['Xi'], c['dt'], record_index=idx, missing='skip')
    npt.assert_allclose(f2, f, rtol=1e-11)
    npt.assert_allclose(g2, g, rtol=0, atol=1e-11 * np.abs(g).max())
    assert F2.shape == (4, 6, 6) and np.isfinite(F2).all()
    assert np.isnan(mle.value_and_grad(pm.build_chirp_model, thetas, recs, c['Xi'], c['dt'], record_index=idx)[0]).all()      # (poison without it)
    with pytest.raises(ValueError, match='missing must be'):
        mle.value_and_grad(pm.build_chirp_model, thetas, recs, c['Xi'], c['dt'], record_index=idx, missing='drop')


def test_mle_standard_errors_on_a_gapped_and_on_an_empty_record():
    """Finite positive standard errors from the `mixed` record's information, equal to the fixture's matrix; a record of NaN only has no
    information: singular, inf everywhere, nll 0."""
    from chirpgp_amd import mle, models as pm
    c = gaps_case(gen.case_name('prefix_ekf', 'mixed'))
    se, cov, info = mle.standard_errors(pm.build_chirp_model, c['theta'], c['ys'], c['Xi'], c['dt'], missing='skip')
    print('standard errors', se, 'cond', info['cond'])
    assert not info['singular'] and np.isfinite(se).all() and (se > 0).all() and np.isfinite(cov).all()
    assert np.abs(info['fisher'] - c['fisher']).max() < FISHER_GATE * np.abs(c['fisher']).max()
    assert abs(info['nll'] - c['nll']) < VALUE_RTOL * abs(c['nll'])
    se, cov, info = mle.standard_errors(pm.build_chirp_model, c['theta'], np.full(130, np.nan), c['Xi'], c['dt'], missing='skip')
    assert info['singular'] and np.isinf(se).all() and np.isinf(cov).all()
    assert info['nll'] == 0.0 and not info['grad'].any() and not info['fisher'].any()


def test_fit_scoring_on_gapped_records():
    """Two gapped T = 130 records, five iterations: every recorded NLL finite and none larger than the one before."""
    from chirpgp_amd import mle, models as pm
    c = grad_case('prefix_ekf')
    recs = np.stack([go.with_gaps(c['ys'], gen.mixed(130)), go.with_gaps(c['ys'], ((20, 50), (100, 130)))])
    opt, info = mle.fit_scoring('ekf', pm.build_chirp_model, [0.1, 0.1, 0.1, 1., 1., 7.], recs, c['Xi'], c['dt'], maxiter=5, missing='skip')
    hist = np.array(info['history'])
    print('history\n', hist)
    assert hist.shape == (info['launches'], 2) and 2 <= info['launches'] <= 6
    assert np.isfinite(hist).all() and np.isfinite(opt).all() and np.isfinite(info['fisher']).all()
    assert np.all(np.diff(hist, axis=0) <= 0)


def test_demo_with_standard_errors_runs(tmp_path):
    out = tmp_path / 'gappy.npz'
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'demos', 'gappy_record.py'), '--T', '600', '--maxiter', '3', '--stderr', '--out', str(out)],
                          check=True, cwd=ROOT, timeout=300, capture_output=True, text=True)
    print(done.stdout)
    assert 'standard errors' in done.stdout and '+-' in done.stdout
    res = np.load(out)
    assert res['standard_errors'].shape == (6,) and res['fisher'].shape == (6, 6)
    npt.assert_array_equal(res['fisher'], res['fisher'].T)
