"""Counterpart of the reference's demos/cd_ghfs_mle.py (BASELINE config C4's driver): continuous-discrete Gauss-Hermite
filter and smoother (RK4 on the sigma-point moment ODEs) on the chirp SDE, parameters by MLE through the filter.

    python demos/cd_ghfs_mle.py [--T 3141] [--seed 555] [--save DIR] [--exact] [--substeps 1] [--maxiter 200]

--exact: the objective's gradient from the continuous-discrete sigma-point tangent kernel (cgp_sgp_nll_grad on the SDE model: forward
tangents through the four RK4 stages of the sigma-point moment ODE and the update, what jax.value_and_grad gives the reference) instead of
13 differenced filter passes.
--substeps n: n RK4 steps of dt / n between two measurements in the objective -- with --exact in its exact gradient too -- and in the
filter and smoother behind the fit.
"""
import argparse

from _pipeline import demo
from chirpgp_amd.quadratures import SigmaPoints

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=3141)
    ap.add_argument('--seed', type=int, default=555)
    ap.add_argument('--save', default=None)
    ap.add_argument('--exact', action='store_true', help='exact gradients (tangent kernel)')
    ap.add_argument('--substeps', type=int, default=1, help='RK4 steps between two measurements (1 .. 16)')
    ap.add_argument('--maxiter', type=int, default=200)
    a = ap.parse_args()
    demo('cd_ghfs', sgps=SigmaPoints.gauss_hermite(d=4, order=3), T=a.T, seed=a.seed, save_dir=a.save, exact=a.exact, substeps=a.substeps,
         maxiter=a.maxiter)
