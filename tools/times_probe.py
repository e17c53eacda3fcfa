"""What per-step intervals cost (`dts=`, include/chirpgp_hip_timed.h): the timed call on a CONSTANT grid, dts = full(T, dt), against the plain
call with that dt -- the same arithmetic per step, so the difference is the delivery of the interval: one 8-byte load per lane and 64-step
chunk, one readlane per step (with substeps one division per lane and chunk more).

    python tools/times_probe.py [--B 512] [--T 50000] [--reps 5] [--n 4] [--untimed-only] [--out profiles/times_probe.txt]

Cases: cd_ekf + cd_eks and GH-3 cd_sgp_filter + cd_sgp_smoother at B x T, cd_ekf alone at 1000 x 10 000 (--ekf-shape).  Times are medians
of --reps launches after one warm-up, taken with device events, with [min .. max].  Prints a table and a sha256 of the untimed outputs (to
compare two commits: they must not move), whether the timed outputs on the constant grid are the untimed ones bit for bit, and writes all of
it to --out.  --untimed-only: a commit without the keyword (the parent of the one that brought it: its untimed times and digests).  Also
times the generic wave kernel (flags CGP_GENERIC_KERNEL | CGP_WAVE_PER_TRIAL) on the timed call at the cd_ekf shape: what a timed call
would run without timed matrix-core kernels; and GH-3 cd_sgp_filter with substeps at --two-waves-shape (2048 x 2000: two wavefronts per SIMD
on 256 CUs), with and without gaps, untimed against timed -- the timed two-pass substep kernels hold one wavefront per SIMD where their untimed
siblings hold two (docs/KERNELS.md).  Gates nothing."""
import argparse
import hashlib
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GENERIC_WAVE = 0x10 | 0x2


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
        del out
    return statistics.median(ms), min(ms), max(ms)


def digest(torch, tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.int64).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=512)
    ap.add_argument('--T', type=int, default=50000)
    ap.add_argument('--ekf-shape', type=int, nargs=2, default=(1000, 10000))
    ap.add_argument('--two-waves-shape', type=int, nargs=2, default=(2048, 2000))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n', type=int, default=4, help='substeps of the flagged rows')
    ap.add_argument('--untimed-only', action='store_true', help='skip dts= (a commit without the keyword)')
    ap.add_argument('--out', default=os.path.join('profiles', 'times_probe.txt'))
    args = ap.parse_args()
    import torch
    from chirpgp_amd import filters_smoothers as fs
    from chirpgp_amd.models import build_chirp_model
    from chirpgp_amd.quadratures import SigmaPoints
    from chirpgp_amd.toymodels import gen_chirp, meow_freq, constant_mag

    drift, disp, _, m0, P0, H = build_chirp_model(np.array([0.1, 0.1, 0.1, 1., 1., 7.]))
    gh3 = SigmaPoints.gauss_hermite(d=4, order=3)
    dt, Xi = 1e-3, 0.1
    lines = [f'# times_probe: B = {args.B}, T = {args.T}, cd_ekf alone at {args.ekf_shape[0]} x {args.ekf_shape[1]}, {args.reps} repetitions (median [min .. max] ms)']

    def record(B, T):
        ts = np.linspace(dt, dt * T, T)
        rng = np.random.default_rng(3)
        clean = gen_chirp(ts, constant_mag(1.), meow_freq(offset=8.)[1])
        return torch.from_numpy(clean[None, :] + np.sqrt(Xi) * rng.standard_normal((B, T))).cuda()

    methods = {
        'cd_ekf': (lambda ys, h, **kw: fs.cd_ekf(drift, disp, H, Xi, m0, P0, h, ys, **kw), lambda mf, Pf, h, **kw: fs.cd_eks(drift, disp, mf, Pf, h, **kw)),
        'cd_sgp': (lambda ys, h, **kw: fs.cd_sgp_filter(drift, disp(None), gh3, H, Xi, m0, P0, h, ys, **kw),
                   lambda mf, Pf, h, **kw: fs.cd_sgp_smoother(drift, disp(None), gh3, mf, Pf, h, **kw)),
    }

    def row(what, t):
        lines.append(f'{what:58s} {t[0]:9.2f} [{t[1]:8.2f} .. {t[2]:8.2f}] ms')
        print(lines[-1], flush=True)

    def note(text):
        lines.append(text)
        print(text, flush=True)

    def same(a, b):
        return all(bool(torch.equal(x.view(torch.int64), y.view(torch.int64))) for x, y in zip(a, b))

    n = args.n
    for name, (B, T, smoother) in (('cd_ekf', (args.B, args.T, True)), ('cd_sgp', (args.B, args.T, True)), ('cd_ekf', (*args.ekf_shape, False))):
        filt, smooth = methods[name]
        ys = record(B, T)
        plain = filt(ys, dt)
        note(f'## {name} {B} x {T}: untimed filter outputs sha256 {digest(torch, plain)}')
        row(f'{name} filter, untimed', timed(torch, lambda: filt(ys, dt), args.reps))
        if smoother:
            note(f'## {name} {B} x {T}: untimed smoother outputs sha256 {digest(torch, smooth(plain[0], plain[1], dt))}')
            row(f'{name} smoother, untimed', timed(torch, lambda: smooth(plain[0], plain[1], dt), args.reps))
        row(f'{name} filter, untimed, substeps={n}', timed(torch, lambda: filt(ys, dt, substeps=n), args.reps))
        if not args.untimed_only:
            dts = torch.full((T,), dt, dtype=torch.float64, device=ys.device)
            note(f'## {name} {B} x {T}: timed filter on the constant grid bit-identical to the untimed one: {same(filt(ys, None, dts=dts), plain)}')
            row(f'{name} filter, dts= (constant grid)', timed(torch, lambda: filt(ys, None, dts=dts), args.reps))
            if smoother:
                note(f'## {name} {B} x {T}: timed smoother bit-identical: {same(smooth(plain[0], plain[1], None, dts=dts), smooth(plain[0], plain[1], dt))}')
                row(f'{name} smoother, dts= (constant grid)', timed(torch, lambda: smooth(plain[0], plain[1], None, dts=dts), args.reps))
            note(f'## {name} {B} x {T}: timed filter with substeps={n} bit-identical: {same(filt(ys, None, dts=dts, substeps=n), filt(ys, dt, substeps=n))}')
            row(f'{name} filter, dts=, substeps={n}', timed(torch, lambda: filt(ys, None, dts=dts, substeps=n), args.reps))
            if not smoother:      # the kernel a timed call would run without the timed matrix-core kernels
                row(f'{name} filter, dts=, generic wave kernel', timed(torch, lambda: filt(ys, None, dts=dts, flags=GENERIC_WAVE), args.reps))
                row(f'{name} filter, untimed, generic wave kernel', timed(torch, lambda: filt(ys, dt, flags=GENERIC_WAVE), args.reps))
        del plain, ys
    # beyond one trial per SIMD: the occupancy of the two-pass (GH-3) sigma-point filter with substeps
    B, T = args.two_waves_shape
    filt = methods['cd_sgp'][0]
    ys = record(B, T)
    gappy = ys.clone()
    gappy[:, 100:140] = float('nan')
    for what, rec, kw in (('', ys, {}), (", missing='skip'", gappy, dict(missing='skip'))):
        row(f'cd_sgp filter {B} x {T}, untimed, substeps={n}{what}', timed(torch, lambda: filt(rec, dt, substeps=n, **kw), args.reps))
        if not args.untimed_only:
            dts = torch.full((T,), dt, dtype=torch.float64, device=ys.device)
            note(f'## cd_sgp {B} x {T}{what}: timed filter with substeps={n} bit-identical: {same(filt(rec, None, dts=dts, substeps=n, **kw), filt(rec, dt, substeps=n, **kw))}')
            row(f'cd_sgp filter {B} x {T}, dts=, substeps={n}{what}', timed(torch, lambda: filt(rec, None, dts=dts, substeps=n, **kw), args.reps))
    del ys, gappy
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
