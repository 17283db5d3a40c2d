"""The Return normaliser's value head (tonic/torch/models/critics.py:17-19 + normalizers/returns.py:19-21) restated
for the tests of the off-policy *_ranged entries: in float32 NumPy in the kernels' operation order (value_squash /
value_squash_dz of csrc/mlpfwd.h) and in float64 torch for autograd.  A helper, not a test."""
import numpy as np

f32 = np.float32


def squash32(z, low, high):
    """v = low + s * t with s = 1 / (1 + exp(-z)), t = high - low: one float32 rounding per operation."""
    z, low, high = np.asarray(z, f32), f32(low), f32(high)
    with np.errstate(over='ignore', invalid='ignore'):
        s = f32(1) / (f32(1) + np.exp(-z, dtype=f32))
        t = f32(high - low)
        return (low + (s * t).astype(f32)).astype(f32)


def squash_dz32(dv, v, low, high):
    """The gradient at z from the gradient dv at v, s recomputed from the published v: s = (v - low) / t, then
    ((dv * t) * (1 - s)) * s — torch's backward of `s * t` followed by sigmoid_backward, left to right."""
    dv, v, low, high = np.asarray(dv, f32), np.asarray(v, f32), f32(low), f32(high)
    with np.errstate(over='ignore', invalid='ignore'):
        t = f32(high - low)
        s = ((v - low).astype(f32) / t).astype(f32)
        return ((((dv * t).astype(f32)) * (f32(1) - s).astype(f32)).astype(f32) * s).astype(f32)


def squash64(z, low, high):
    """float64 torch, differentiable: what ValueHead.forward + Return.forward compute."""
    import torch
    low, high = float(low), float(high)
    return low + torch.sigmoid(z) * (high - low)


def ulps(got, want):
    """Distance in float32 units in the last place of `want` (inf where exactly one of the two is not finite)."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    spacing = np.spacing(np.abs(want).astype(f32)).astype(np.float64)
    with np.errstate(invalid='ignore'):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / spacing
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    return np.where(same, 0.0, np.where(np.isfinite(d), d, np.inf))
