"""Run-time compiled models (cgp_model_from_source; csrc/cgp_custom.hpp, csrc/cgp_rtc.hip) against 100-digit arithmetic, the GPU half.

1. The operation table (tests/golden/exact_custom_ops.npz): every overload of cgp::ad::Dual<N> as one trial's measurement function, one
   step of ekf_for_kpt, d = 3 and d = 8 -- one compilation and one launch per dimension -- each trial against its exact (mf, Pf, nll).
2. The ring (exact_custom_ring.npz): one model family at every dimension the C entry point accepts, d = 1 .. 8, through all eight methods.
3. Batching and edges of the custom launch path at d = 5.
The gates are tests/test_exact_custom.py's: set by the NumPy oracle's measured distance from the same exact values, not by the kernels'."""
import time

import numpy as np
import pytest

from tests import cases as cs
from tests import custom_exact as cx
from tests import test_exact_custom as tx

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('d', [3, 8])
def test_every_dual_number_operation_against_its_exact_value(d):
    from chirpgp_amd import filters_smoothers as fs, models as pm
    z = tx.load('exact_custom_ops')
    F, Sigma, P0, Xi = z[f'd{d}.F'], z[f'd{d}.Sigma'], z[f'd{d}.P0'], float(z[f'd{d}.Xi'])
    h = pm.custom_measurement(cx.ops_source(d), d, z[f'd{d}.q'])
    ys = z[f'd{d}.y'][:, None]
    mfs, Pfs, nll = fs.ekf_for_kpt(F, Sigma, h, Xi, z[f'd{d}.m0'], P0, 0.0, ys)
    tx.check_ops(z, d, (mfs[:, 0], Pfs[:, 0], nll[:, 0]), 'hip')
    last = fs.ekf_for_kpt(F, Sigma, h, Xi, z[f'd{d}.m0'], P0, 0.0, ys, nll_final_only=True, want=(False, False, True))
    assert last[0] is None and last[1] is None and np.array_equal(last[2], nll[:, 0], equal_nan=True)


# ------------------------------------------------------------------------------------------------ the ring
def ring_models(d, p, b):
    from chirpgp_amd import models as pm
    disc = pm.custom_cond_m_cov(cx.ring_source(d), d, p)
    sde, disp = pm.custom_sde(cx.ring_source(d), d, p, b)
    return disc, sde, disp


def ring_hip(disc, sde, disp, b, sg, H, Xi, m0, P0, dt, ys, methods=cx.METHODS, rows=None, **kw):
    """the methods of `methods` on the compiled ring; a smoother is fed rows(its filter's name) if given, else that filter's own rows"""
    from chirpgp_amd import filters_smoothers as fs
    out = {}
    feed = (lambda fn: rows(fn)) if rows is not None else (lambda fn: out[fn][:2])
    run = {'ekf': lambda: fs.ekf(disc, H, Xi, m0, P0, dt, ys, **kw), 'eks': lambda: fs.eks(disc, *feed('ekf'), dt),
           'sgp_filter': lambda: fs.sgp_filter(disc, sg, H, Xi, m0, P0, dt, ys, **kw), 'sgp_smoother': lambda: fs.sgp_smoother(disc, sg, *feed('sgp_filter'), dt),
           'cd_ekf': lambda: fs.cd_ekf(sde, disp, H, Xi, m0, P0, dt, ys, **kw), 'cd_eks': lambda: fs.cd_eks(sde, disp, *feed('cd_ekf'), dt),
           'cd_sgp_filter': lambda: fs.cd_sgp_filter(sde, b, sg, H, Xi, m0, P0, dt, ys, **kw),
           'cd_sgp_smoother': lambda: fs.cd_sgp_smoother(sde, b, sg, *feed('cd_sgp_filter'), dt)}
    for fn in methods:
        out[fn] = run[fn]()
    return out


@pytest.mark.parametrize('d', range(1, 9))
def test_the_ring_model_at_every_dimension_through_all_eight_methods(d):
    """Dual<d>, CustomDisc / CustomSDE, sgp_prediction_literal and CdSgpPredict<CustomSDE> instantiated at d; the smoothers on the rounded
    exact filtering rows.  Prints what the two compilations took."""
    from chirpgp_amd import _engine
    z = tx.load('exact_custom_ring')
    i_ = tx.ring_inputs(z, d)
    disc, sde, disp = ring_models(d, i_['p'], i_['b'])
    t0 = time.perf_counter()
    _engine.custom_model(disc)
    t1 = time.perf_counter()
    _engine.custom_model(sde)
    print(f'ring d = {d}: compiled the discrete model in {t1 - t0:.2f} s, the SDE model in {time.perf_counter() - t1:.2f} s')
    for pre, sg, methods in tx.ring_sets(d):
        got = ring_hip(disc, sde, disp, i_['b'], sg, i_['H'], float(i_['Xi']), i_['m0'], i_['P0'], float(i_['dt']), i_['ys'], methods,
                       rows=lambda fn: (z[f'{pre}{fn}.0'], z[f'{pre}{fn}.1']))
        tx.check_ring(z, d, pre, methods, got, 'hip')


# ------------------------------------------------------------------------------------------------ batching and edges, d = 5
D5, T5, BMAX = 5, 20, 130


class Batch:
    """BMAX trials of the ring at d = 5, everything per trial: p, m0, P0, H, Xi, ys"""
    def __init__(self):
        from chirpgp_amd.quadratures import SigmaPoints
        rng = np.random.default_rng(55)
        d = D5
        self.p = np.array([0.8, 0.6, 0.3, 0.05, 0.4]) * rng.uniform(0.8, 1.25, (BMAX, 5))
        self.b = 0.3 * np.eye(d) + 0.15 * rng.standard_normal((d, d))
        self.H = rng.uniform(0.4, 1.0, (BMAX, d)) * rng.choice([-1.0, 1.0], (BMAX, d))
        self.Xi = rng.uniform(0.2, 0.5, BMAX)
        self.m0 = 0.6 * rng.standard_normal((BMAX, d))
        A = 0.3 * rng.standard_normal((BMAX, d, d))
        self.P0 = A @ np.transpose(A, (0, 2, 1)) + 0.2 * np.eye(d)
        self.ys = rng.standard_normal((BMAX, T5))
        self.dt = 0.05
        self.sg = SigmaPoints.cubature(d)

    def run(self, sel, ys=None, methods=cx.METHODS, **kw):
        """sel: a slice (a batch) or an int (a single record: every operand loses its leading axis)"""
        disc, sde, disp = ring_models(D5, self.p[sel], self.b)
        return ring_hip(disc, sde, disp, self.b, self.sg, self.H[sel], self.Xi[sel], self.m0[sel], self.P0[sel], self.dt,
                        self.ys[sel] if ys is None else ys, methods, **kw)


@pytest.fixture(scope='module')
def batch():
    bt = Batch()
    bt.full = bt.run(slice(0, BMAX))
    return bt


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_every_trial_of_a_batch_is_its_own_single_record_run_bit_for_bit(batch):
    """One lane per trial, no cross-lane arithmetic: a trial's numbers do not depend on the batch around it.  B = 130 against 130
    single-record runs; B = 1, 63, 64, 65 (a ragged last wavefront, an exact one, one trial past it) are leading trials of the same batch."""
    assert all(np.all(np.isfinite(a)) for v in batch.full.values() for a in v)
    for i in range(BMAX):
        one = batch.run(i)
        for fn in cx.METHODS:
            assert one[fn][0].shape == (T5, D5)
            assert same(one[fn], [a[i] for a in batch.full[fn]]), (fn, i)
    for B in (1, 63, 64, 65):
        got = batch.run(slice(0, B))
        for fn in cx.METHODS:
            assert got[fn][0].shape == (B, T5, D5) and same(got[fn], [a[:B] for a in batch.full[fn]]), (fn, B)


def test_a_few_trials_of_the_batch_against_the_numpy_oracle(batch):
    """... and the batch is right, not only self-consistent: both sit within the method's gate of the exact value, so within twice the
    gate of each other (T = 20 against the fixture's 8: the first 8 steps)."""
    from oracle import np_filters as onf
    osg = cs.osig(batch.sg)
    for i in (0, 63, 64, 129):
        drift, cond = cx.ring_host(batch.p[i])
        a = (batch.H[i], batch.Xi[i], batch.m0[i], batch.P0[i], batch.dt, batch.ys[i, :8])
        want = {'ekf': onf.ekf(cond, *a), 'sgp_filter': onf.sgp_filter(cond, osg, *a), 'cd_ekf': onf.cd_ekf(drift, lambda _: batch.b, *a),
                'cd_sgp_filter': onf.cd_sgp_filter(drift, batch.b, osg, *a)}
        for fn, w in want.items():
            assert tx.distance([g[i, :8] for g in batch.full[fn]], w) < 2 * tx.GATE_RING[fn], (fn, i)


def test_records_of_one_and_two_steps(batch):
    from oracle import np_filters as onf
    osg = cs.osig(batch.sg)
    for T in (1, 2):
        got = batch.run(slice(0, 3), ys=batch.ys[:3, :T])
        for f, s in zip(cx.METHODS[::2], cx.METHODS[1::2]):
            assert got[f][0].shape == (3, T, D5) and got[f][2].shape == (3, T) and got[s][1].shape == (3, T, D5, D5)
            assert same(got[f], [a[:3, :T] for a in batch.full[f]]), (f, T)            # a filter is causal
            assert same([g[:, -1] for g in got[s]], [g[:, -1] for g in got[f][:2]]), (s, T)      # the last smoothing row is the filtering row
    # T = 2: the one smoothing step against the oracle on the same filtering rows, within twice the gate (each within the gate of exact)
    i = 1
    drift, cond = cx.ring_host(batch.p[i])
    want = {'eks': onf.eks(cond, got['ekf'][0][i], got['ekf'][1][i], batch.dt), 'sgp_smoother': onf.sgp_smoother(cond, osg, got['sgp_filter'][0][i], got['sgp_filter'][1][i], batch.dt),
            'cd_eks': onf.cd_eks(drift, lambda _: batch.b, got['cd_ekf'][0][i], got['cd_ekf'][1][i], batch.dt),
            'cd_sgp_smoother': onf.cd_sgp_smoother(drift, batch.b, osg, got['cd_sgp_filter'][0][i], got['cd_sgp_filter'][1][i], batch.dt)}
    for fn, w in want.items():
        assert tx.distance([g[i] for g in got[fn]], w) < 2 * tx.GATE_RING[fn], fn


def test_empty_batches_and_empty_records(batch):
    for B, T in ((0, T5), (3, 0)):
        got = batch.run(slice(0, B), ys=batch.ys[:B, :T])
        for f, s in zip(cx.METHODS[::2], cx.METHODS[1::2]):
            assert [a.shape for a in got[f]] == [(B, T, D5), (B, T, D5, D5), (B, T)], (f, B, T)
            assert [a.shape for a in got[s]] == [(B, T, D5), (B, T, D5, D5)], (s, B, T)


def test_partial_outputs_are_the_full_runs_numbers(batch):
    filters = cx.METHODS[::2]
    for want in ((True, False, True), (False, False, True)):
        got = batch.run(slice(0, 65), methods=filters, want=want)
        for fn in filters:
            for k in range(3):
                assert (got[fn][k] is None) == (not want[k])
                assert got[fn][k] is None or np.array_equal(got[fn][k], batch.full[fn][k][:65]), (fn, want, k)


def test_a_nan_measurement_stays_in_its_trial(batch):
    """tests/test_gpu_parity.py:test_nan_semantics for the custom kernels: NaN exactly where the oracle has NaN, no exception, and every other
    trial untouched.  The update's Pf does not read y, so step k keeps its covariance; the next prediction linearises at a NaN mean."""
    from oracle import np_filters as onf
    osg = cs.osig(batch.sg)
    B, i, k = 65, 64, 7
    ys = batch.ys[:B].copy()
    ys[i, k] = np.nan
    filters = cx.METHODS[::2]
    got = batch.run(slice(0, B), ys=ys, methods=filters)
    drift, cond = cx.ring_host(batch.p[i])
    a = (batch.H[i], batch.Xi[i], batch.m0[i], batch.P0[i], batch.dt, ys[i])
    want = {'ekf': onf.ekf(cond, *a), 'sgp_filter': onf.sgp_filter(cond, osg, *a), 'cd_ekf': onf.cd_ekf(drift, lambda _: batch.b, *a),
            'cd_sgp_filter': onf.cd_sgp_filter(drift, batch.b, osg, *a)}
    others = np.arange(B) != i
    for fn in filters:
        mfs, Pfs, nll = got[fn]
        assert np.all(np.isnan(mfs[i, k:])) and np.all(np.isnan(nll[i, k:])) and np.all(np.isnan(Pfs[i, k + 1:])) and np.all(np.isfinite(Pfs[i, k])), fn
        for g, w, full in zip(got[fn], want[fn], batch.full[fn]):
            assert np.array_equal(np.isnan(g[i]), np.isnan(w)), fn
            assert np.array_equal(g[i, :k], full[i, :k]) and np.array_equal(g[others], full[:B][others]), fn
        assert np.array_equal(Pfs[i, k], batch.full[fn][1][i, k]), fn


def test_torch_tensors_in_torch_tensors_out(batch):
    import torch
    B = 65
    ys = torch.from_numpy(batch.ys[:B]).cuda()
    got = batch.run(slice(0, B), ys=ys)
    for fn in cx.METHODS:
        for g, full in zip(got[fn], batch.full[fn]):
            assert torch.is_tensor(g) and g.device == ys.device and g.dtype == torch.float64, fn
            assert np.array_equal(g.cpu().numpy(), full[:B]), fn


M_SIN = 'template <class T> __device__ T measure(const T* u, const double* q) { return sin(u[0]) * u[1] + q[0] * u[2]; }\n'
M_COS = 'template <class T> __device__ T measure(const T* u, const double* q) { return cos(u[0]) * u[1] - q[0] * u[2]; }\n'


def test_live_models_do_not_leak_into_each_other_and_come_back_after_release(batch):
    """The same source at d = 4 and d = 5 and two sources at d = 5, all loaded at once and called in turn; then every code object unloaded
    and the batch run again.  (The bound against the oracle is not an accuracy gate -- another model's code is an O(1) difference.)"""
    from chirpgp_amd import _engine, filters_smoothers as fs, models as pm
    from oracle import np_filters as onf
    rng = np.random.default_rng(9)
    q = np.array([0.7])
    hosts = {M_SIN: lambda u: np.sin(u[0]) * u[1] + q[0] * u[2], M_COS: lambda u: np.cos(u[0]) * u[1] - q[0] * u[2]}
    jobs = []
    for src, d in ((M_SIN, 4), (M_SIN, 5), (M_COS, 5)):
        F = np.eye(d) + 0.05 * rng.standard_normal((d, d))
        A = 0.3 * rng.standard_normal((d, d))
        jobs.append((src, d, (F, A @ A.T + 0.05 * np.eye(d)), (0.3, 0.5 * rng.standard_normal(d), np.eye(d), 0.0, rng.standard_normal(T5))))
    first = [fs.ekf_for_kpt(*lin, pm.custom_measurement(src, d, q), *rest) for src, d, lin, rest in jobs]
    for (src, d, lin, rest), got in zip(jobs, first):
        again = fs.ekf_for_kpt(*lin, pm.custom_measurement(src, d, q), *rest)
        assert got[0].shape == (T5, d) and same(got, again), (d, src)
        assert tx.distance(got, onf.ekf_for_kpt(*lin, hosts[src], *rest)) < 1e4, (d, src)
    assert _engine.release_custom_models() >= 5 and _engine.release_custom_models() == 0
    again = batch.run(slice(0, BMAX))
    for fn in cx.METHODS:
        assert same(again[fn], batch.full[fn]), fn
