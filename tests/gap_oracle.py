"""The NumPy oracle with missing measurements (missing='skip', CGP_SKIP_MISSING): at a step whose measurement is NaN the prediction is the
filtering result and the NLL increment is exactly 0.

Nine of the ten oracle filters update through oracle.np_filters._linear_update, so the gapped oracle IS the oracle, run with that one
function replaced: (mp, Pp, 0.0) for a NaN measurement, the original otherwise.  ekf_for_kpt has its update inline; its one step is
restated here from the oracle's own pieces.  tests/test_gap_oracle.py checks the construction against dense Gaussian conditioning on the
observed samples."""
from unittest import mock

import numpy as np

from oracle import np_filters as onp

_linear_update = onp._linear_update


def _gapped_linear_update(mp, Pp, H, Xi, y):
    if np.isnan(y):                                    # the measurement alone decides: never the innovation, never S
        return mp, Pp, 0.0
    return _linear_update(mp, Pp, H, Xi, y)


def gapped(fn, *args):
    """An oracle filter of np_filters (kf, ekf, cd_ekf, sgp_filter, cd_sgp_filter) with NaN measurements skipped."""
    assert fn is not onp.ekf_for_kpt, 'ekf_for_kpt updates inline: gapped_ekf_for_kpt'
    with mock.patch.object(onp, '_linear_update', _gapped_linear_update):
        return fn(*args)


def gapped_ekf_for_kpt(F, Sigma, h, Xi, m0, P0, dt, ys):
    """np_filters.ekf_for_kpt (filters_smoothers.py:267-314) with NaN measurements skipped."""
    def step(mf, Pf, y):
        mp, Pp = onp._linear_predict(F, Sigma, mf, Pf)
        if np.isnan(y):
            return mp, Pp, 0.0
        H = onp.jacobian(lambda x: np.atleast_1d(h(x)), mp)[0]
        S = H @ Pp @ H.T + Xi
        K = Pp @ H.T / S
        pred = h(mp)
        return mp + K * (y - pred), Pp - np.outer(K, K) * S, onp._neg_log_normal_pdf(y, pred, S)
    return onp._run_filter(step, m0, P0, ys)


def with_gaps(ys, spans, shift=0):
    """A copy of the record with NaN over the half-open step ranges `spans`, each moved by `shift` steps (clipped to the record)."""
    out = np.array(ys, dtype=np.float64)
    for a, b in spans:
        out[max(a + shift, 0):max(min(b + shift, out.size), 0)] = np.nan
    return out
