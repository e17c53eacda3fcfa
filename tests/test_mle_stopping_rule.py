"""The stopping rule of chirpgp_amd.mle.fit where it differences the filter's NLL (mle.DIFFERENCE_STOP), on the C port's objective (no
GPU): the likelihood of a chirp record ends in a shallow valley, and a rule as loose as SciPy's default lets the last bits of the NLL
decide where in it the search stops -- any re-ordering of a filter kernel's arithmetic then moves the reported parameters.  The rule
must make the stopping point a property of the record: NLL values perturbed by a few units in the last place (2e-14 relative, what the
engine's kernels differ by among themselves and from the port) have to lead to the same parameters well inside the 1e-3 to which
tests/test_gpu_mle_oracle.py holds the driver against the port's tightly converged optimum."""
import numpy as np

from tests import mle_oracle as mo
from tests.test_gpu_mle_oracle import _record, INIT

KEEP = np.array([0, 2, 3, 4, 5])            # (`b` is driven to zero on these records: a flat direction, compared absolutely there)


def _objective(ys, noise, seed, rel_step=1e-6):
    """mle.make_objective's difference form on the port: 13 probes, central differences; every NLL perturbed by `noise` relative."""
    from chirpgp_amd import models as pm
    rng = np.random.default_rng(seed)

    def fun(theta):
        P = theta.size
        h = rel_step * (1.0 + np.abs(theta))
        batch = np.tile(theta, (2 * P + 1, 1))
        for i in range(P):
            batch[1 + 2 * i, i] += h[i]
            batch[2 + 2 * i, i] -= h[i]
        nll = mo.nll('ekf', pm.build_chirp_model, batch, ys, 0.1, 1e-3)
        nll = nll * (1.0 + noise * rng.standard_normal(nll.shape))
        return float(nll[0]), (nll[1::2] - nll[2::2]) / (2 * h)
    return fun


def test_last_bits_of_the_nll_do_not_move_the_reported_optimum():
    from scipy.optimize import minimize
    from chirpgp_amd import mle, models as pm
    ys = _record(3141, 555)
    opt_o, _ = mo.fit('ekf', pm.build_chirp_model, INIT, ys, 0.1, 1e-3)
    far = {}
    for label, stop in (('SciPy default', {}), ('mle.DIFFERENCE_STOP', mle.DIFFERENCE_STOP)):
        opts = [mo.g(minimize(_objective(ys, 2e-14, seed), mo.g_inv(INIT), jac=True, method='L-BFGS-B', options=dict(maxiter=300, **stop)).x)
                for seed in (1, 2, 3, 4)]
        far[label] = [float(np.abs(o[KEEP] / opt_o[KEEP] - 1).max()) for o in opts]
        print(label, 'largest relative distance from the tight optimum, four perturbed runs:', ['%.1e' % e for e in far[label]])
    # a fifth of the gate: the rule may use up some of the 1e-3, not most of it (the default rule, printed above, reaches 2e-3)
    assert max(far['mle.DIFFERENCE_STOP']) <= 2e-4, far
