"""tests/golden/exact_gaps_grad.npz (tests/golden/make_exact_gaps_grad.py): the 100-digit value, gradient and Fisher information of records
with gaps that tests/test_gpu_gaps_gradient.py holds the four tangent entry points to.  Here, without a GPU: the file holds what the
generator's list says under the generator's admission rule, and every case's value is the float64 oracle's with NaN measurements skipped
(tests/gap_oracle.py, the construction that pins the filters) at 1e-9 -- the gaps tests' own gate."""
import numpy as np
import pytest

from tests import cases as cs
from tests import gap_oracle as go
from tests.gaps_grad_cases import ZGAPS, gaps_case, NAMES
from tests.golden import make_exact_gaps_grad as gen

GATE = 1e-9


def test_counts_and_admission_rule():
    """At least 22 of the generator's 26 cases and one of every line; every kept case moved by less than the rule allows (the edge_* cases
    are exempt and carry their movement); what was rejected is listed with its movement."""
    listed = [gen.case_name(s, p) for line in gen.CASES for s, p in line]
    assert len(listed) == 26 and [len(line) for line in gen.CASES] == [14, 5, 4, 2, 1]
    rejected = [str(n) for n in ZGAPS['rejected']]
    assert sorted(NAMES + rejected) == sorted(listed)
    assert ZGAPS['rejected_moved'].shape == (len(rejected), 3)
    assert len(NAMES) >= gen.MIN_CASES == 22
    for line in gen.CASES:
        assert {gen.case_name(s, p) for s, p in line} & set(NAMES), line
    for n in NAMES:
        c = gaps_case(n)
        moved = (c['moved_nll'], c['moved_grad'], c['moved_fisher'])
        assert all(np.isfinite(moved)), (n, moved)
        if not c['source'].startswith('edge_'):
            assert moved[0] < 1e-13 and moved[1] < 1e-10 and moved[2] < 1e-10, (n, moved)
        nd = c['n_dir']
        assert c['grad'].shape == (nd,) and c['fisher'].shape == (nd, nd) and np.isfinite(c['fisher']).all() and np.isfinite(c['grad']).all()
        assert c['n_observed'] == int(np.isfinite(c['ys']).sum()) >= 1
        want = np.array(c['src_ys'])                                     # the source's record with NaN over the stored ranges, nothing else
        for a, b in c['gaps']:
            want[a:b] = np.nan
        np.testing.assert_array_equal(c['ys'], want)


def test_the_case_without_a_gap_is_the_source_case():
    c = gaps_case(gen.case_name('prefix_ekf', 'none'))
    from tests.tangent_cases import ZF, ZG
    assert c['nll'] == float(ZG['prefix_ekf.nll'])
    np.testing.assert_array_equal(c['grad'], ZG['prefix_ekf.grad'])
    np.testing.assert_array_equal(c['fisher'], ZF['prefix_ekf.fisher'])


@pytest.mark.parametrize('name', NAMES)
def test_value_against_the_gapped_oracle(name):
    """The final NLL of oracle ekf / sgp_filter with NaN measurements skipped, float64, within 1e-9 of the 100-digit value."""
    from chirpgp_amd import models as pm
    from oracle import np_filters as onp, np_models as om
    from tests.tangent_cases import sigma
    c = gaps_case(name)
    with np.errstate(all='ignore'):
        params = pm.g(c['theta'])
        _, _, o_disc, m0, P0, _ = (om.build_chirp_model if c['build'] == 'chirp' else om.build_lascala_model)(params)
    if c['method'] == 'ekf':
        got = go.gapped(onp.ekf, o_disc, c['H'], c['Xi'], m0, P0, c['dt'], c['ys'])[2][-1]
    else:
        got = go.gapped(onp.sgp_filter, o_disc, cs.osig(sigma(c['sigma'])), c['H'], c['Xi'], m0, P0, c['dt'], c['ys'])[2][-1]
    err = abs(got - c['nll']) / abs(c['nll'])
    print(f'{name}: oracle {got!r}, exact {c["nll"]!r}, {err:.2e}')
    assert err <= GATE, (got, c['nll'])
