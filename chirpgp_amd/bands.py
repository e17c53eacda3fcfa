"""Credible bands from posterior sample paths (filters_smoothers.eks_sample and its siblings): torch on the paths' own device."""
import math

__all__ = ['pointwise_band', 'simultaneous_band']


def _paths(comp_paths):
    import torch
    t = comp_paths if isinstance(comp_paths, torch.Tensor) else torch.as_tensor(comp_paths)
    if t.ndim < 2:
        raise ValueError(f'comp_paths must be (S, T) or (B, S, T); got {tuple(t.shape)}')
    if t.shape[-2] < 2:
        raise ValueError('a band needs at least two sample paths')
    return t.to(torch.float64)


def pointwise_band(comp_paths, level=0.95):
    """mean -+ z sd per step, z the two-sided normal quantile of `level`: each step alone is covered with probability `level`.
    comp_paths (S, T) or (B, S, T) -> (lo, hi, z), lo and hi (T,) or (B, T)."""
    import torch
    x = _paths(comp_paths)
    z = math.sqrt(2.0) * float(torch.erfinv(torch.tensor(float(level), dtype=torch.float64)))
    mean, sd = x.mean(dim=-2), x.std(dim=-2)
    return mean - z * sd, mean + z * sd, z


def simultaneous_band(comp_paths, level=0.95):
    """The smallest k such that a fraction `level` of the paths stay inside mean -+ k sd at EVERY step (the `level` quantile of the
    paths' largest standardised deviation): a band for the whole track, not for one step.  A step without spread (sd = 0) deviates by 0.
    comp_paths (S, T) or (B, S, T) -> (lo, hi, k), lo and hi (T,) or (B, T), k a float or (B,)."""
    import torch
    if not 0.0 < float(level) <= 1.0:
        raise ValueError('level must be in (0, 1]')
    x = _paths(comp_paths)
    S = x.shape[-2]
    mean, sd = x.mean(dim=-2, keepdim=True), x.std(dim=-2, keepdim=True)
    dev = torch.where(sd > 0, (x - mean).abs() / torch.where(sd > 0, sd, torch.ones_like(sd)), torch.zeros_like(x))
    worst = dev.amax(dim=-1)                                    # (.., S): every path's largest deviation
    need = min(S, max(1, math.ceil(float(level) * S - 1e-12)))  # paths that must stay inside
    k = worst.sort(dim=-1).values[..., need - 1]
    kk = k[..., None]
    lo, hi = mean.squeeze(-2) - kk * sd.squeeze(-2), mean.squeeze(-2) + kk * sd.squeeze(-2)
    return lo, hi, (float(k) if k.ndim == 0 else k)
