"""What RK4 substeps cost (CGP_RK4_SUBSTEPS, `substeps=n`): in-kernel against the gap emulation of the same n -- the record refined n times
with NaN at the inserted times, missing='skip' at dt / n, every n-th row kept -- and the unflagged call beside them.

    python tools/substeps_probe.py [--B 512] [--T 50000] [--reps 5] [--ns 2 4 8] [--no-in-kernel] [--no-emulation] [--out profiles/substeps_probe.txt]

Cases: cd_ekf + cd_eks and GH-3 cd_sgp_filter + cd_sgp_smoother at B x T, cd_ekf alone at 1000 x 10 000 (--ekf-shape).  Times are medians
of --reps launches after one warm-up, taken with device events; memory is torch's peak allocation over one pass (outputs included, which
is the point: the emulation's are n times the size).  Prints a table and a sha256 of the unflagged outputs (to compare two commits), and
writes both to --out.  --no-in-kernel: a commit without the keyword (the parent of the one that brought it: its unflagged times and
digests, and the emulation, which is that commit's way to substeps).  Gates nothing."""
import argparse
import hashlib
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def peak(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    got = torch.cuda.max_memory_allocated() - base
    del out
    return got / 2 ** 20


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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ns', type=int, nargs='*', default=[2, 4, 8])
    ap.add_argument('--no-in-kernel', action='store_true', help='skip substeps=n (a commit without the keyword)')
    ap.add_argument('--no-emulation', action='store_true', help='skip the gap emulation')
    ap.add_argument('--out', default=os.path.join('profiles', 'substeps_probe.txt'))
    args = ap.parse_args()
    import torch
    from chirpgp_amd import filters_smoothers as fs
    from chirpgp_amd.models import build_chirp_model
    from chirpgp_amd.quadratures import SigmaPoints
    from chirpgp_amd.toymodels import gen_chirp, meow_freq, constant_mag

    drift, disp, _, m0, P0, H = build_chirp_model(np.array([0.1, 0.1, 0.1, 1., 1., 7.]))
    gh3 = SigmaPoints.gauss_hermite(d=4, order=3)
    dt, Xi = 1e-3, 0.1
    lines = [f'# substeps_probe: B = {args.B}, T = {args.T}, cd_ekf alone at {args.ekf_shape[0]} x {args.ekf_shape[1]}, {args.reps} repetitions (median [min .. max] ms)']

    def record(B, T):
        ts = np.linspace(dt, dt * T, T)
        rng = np.random.default_rng(3)
        clean = gen_chirp(ts, constant_mag(1.), meow_freq(offset=8.)[1])
        return torch.from_numpy(clean[None, :] + np.sqrt(Xi) * rng.standard_normal((B, T))).cuda()

    def refined(ys, n):
        ref = torch.full((ys.shape[0], n * ys.shape[1]), float('nan'), dtype=torch.float64, device=ys.device)
        ref[:, n - 1::n] = ys
        return ref

    methods = {
        'cd_ekf': (lambda ys, h, **kw: fs.cd_ekf(drift, disp, H, Xi, m0, P0, h, ys, **kw), lambda mf, Pf, h, **kw: fs.cd_eks(drift, disp, mf, Pf, h, **kw)),
        'cd_sgp': (lambda ys, h, **kw: fs.cd_sgp_filter(drift, disp(None), gh3, H, Xi, m0, P0, h, ys, **kw),
                   lambda mf, Pf, h, **kw: fs.cd_sgp_smoother(drift, disp(None), gh3, mf, Pf, h, **kw)),
    }

    def row(what, t, mem):
        lines.append(f'{what:58s} {t[0]:9.2f} [{t[1]:8.2f} .. {t[2]:8.2f}] ms   peak {mem:9.1f} MiB')
        print(lines[-1], flush=True)

    for name, (B, T, smoother) in (('cd_ekf', (args.B, args.T, True)), ('cd_sgp', (args.B, args.T, True)), ('cd_ekf', (*args.ekf_shape, False))):
        filt, smooth = methods[name]
        ys = record(B, T)
        plain = filt(ys, dt)
        lines.append(f'## {name} {B} x {T}: unflagged outputs sha256 {digest(torch, plain)}')
        print(lines[-1], flush=True)
        row(f'{name} filter, unflagged', timed(torch, lambda: filt(ys, dt), args.reps), peak(torch, lambda: filt(ys, dt)))
        if smoother:
            row(f'{name} smoother, unflagged', timed(torch, lambda: smooth(plain[0], plain[1], dt), args.reps), peak(torch, lambda: smooth(plain[0], plain[1], dt)))
        del plain
        for n in args.ns:
            if not args.no_in_kernel:
                inside = filt(ys, dt, substeps=n)
                row(f'{name} filter, substeps={n}', timed(torch, lambda: filt(ys, dt, substeps=n), args.reps), peak(torch, lambda: filt(ys, dt, substeps=n)))
                if smoother:
                    row(f'{name} smoother, substeps={n}', timed(torch, lambda: smooth(inside[0], inside[1], dt, substeps=n), args.reps),
                        peak(torch, lambda: smooth(inside[0], inside[1], dt, substeps=n)))
                del inside
            if not args.no_emulation:
                ref = refined(ys, n)
                row(f'{name} filter, gap emulation n={n}', timed(torch, lambda: filt(ref, dt / n, missing='skip'), args.reps),
                    peak(torch, lambda: filt(ref, dt / n, missing='skip')))
                if smoother:
                    full = filt(ref, dt / n, missing='skip')
                    row(f'{name} smoother, gap emulation n={n}', timed(torch, lambda: smooth(full[0], full[1], dt / n), args.reps),
                        peak(torch, lambda: smooth(full[0], full[1], dt / n)))
                    del full
                del ref
        del ys
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
