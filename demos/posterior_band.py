"""Credible bands for the instantaneous frequency from posterior sample paths: one record of demos/ekfs_mle.py's setup (the constant-
magnitude chirp, the model at the MLE start point), EKF -> eks_sample(select = softplus of the frequency state) -> bands.

    python demos/posterior_band.py [--T 3141] [--samples 1024] [--level 0.95] [--seed 555] [--gaps]

The pointwise band covers each step with probability `level`; the simultaneous band (bands.simultaneous_band) covers the WHOLE track
with that probability, which takes the joint law of the path -- backward simulation on the smoother's own maps (cgp_smoother_sample).
The script reports the share of the true frequency track inside each band.
--gaps: blanks a segment in the middle and the last fifth of the record (missing='skip'): over the tail the paths are a forecast
ensemble, and the band opens with the horizon.
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chirpgp_amd import filters_smoothers as fs                                       # noqa: E402
from chirpgp_amd.bands import pointwise_band, simultaneous_band                       # noqa: E402
from chirpgp_amd.models import build_chirp_model                                      # noqa: E402
from chirpgp_amd.toymodels import gen_chirp, meow_freq, constant_mag                  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=3141)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--level', type=float, default=0.95)
    ap.add_argument('--seed', type=int, default=555)
    ap.add_argument('--gaps', action='store_true', help='blank a segment and the tail: a forecast ensemble')
    args = ap.parse_args(argv)

    dt, T, Xi = 0.001, args.T, 0.1
    ts = np.linspace(dt, dt * T, T)
    rng = np.random.default_rng(args.seed)
    true_freq_func, true_phase_func = meow_freq(offset=8.)
    ys = gen_chirp(ts, constant_mag(1.), true_phase_func) + math.sqrt(Xi) * rng.standard_normal(T)
    observed = np.ones(T, dtype=bool)
    if args.gaps:
        observed[2 * T // 5:T // 2] = False
        observed[4 * T // 5:] = False
        ys = np.where(observed, ys, np.nan)

    _, _, m_and_cov, m0, P0, H = build_chirp_model(np.array([0.1, 0.1, 0.1, 1., 1., 7.]))
    mfs, Pfs, _ = fs.ekf(m_and_cov, H, Xi, m0, P0, dt, ys, **(dict(missing='skip') if args.gaps else {}))
    _, freq = fs.eks_sample(m_and_cov, mfs, Pfs, dt, args.samples, seed=args.seed, want_paths=False, select=dict(comp=2, func='softplus'))

    truth = true_freq_func(ts)
    out = {'level': args.level, 'samples': args.samples}
    for name, (lo, hi, k) in (('pointwise', pointwise_band(freq, args.level)), ('simultaneous', simultaneous_band(freq, args.level))):
        lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
        inside = (truth >= lo) & (truth <= hi)
        out[name] = dict(k=float(k), coverage=float(inside.mean()), width=float((hi - lo).mean()), lo=lo, hi=hi)
        line = f'{name:13s} mean +- {float(k):.2f} sd   mean width {out[name]["width"]:.3f} Hz   true track inside at {100 * inside.mean():.1f} % of the steps'
        if args.gaps:
            tail = slice(4 * T // 5, T)
            out[name]['tail_coverage'] = float(inside[tail].mean())
            out[name]['tail_width'] = (float((hi - lo)[tail][0]), float((hi - lo)[tail][-1]))
            line += f'   forecast tail: {100 * inside[tail].mean():.1f} %, width {out[name]["tail_width"][0]:.3f} -> {out[name]["tail_width"][1]:.3f} Hz'
        print(line)
    return out


if __name__ == '__main__':
    main()
