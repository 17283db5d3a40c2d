"""The float32 statement of the critic-loss rules (tonic_critic_loss_t, include/tonic_hip.h) in NumPy: what
critic_loss_term / critic_loss_dq of csrc/mlpfwd.h compute on an error e = q - y, operation for operation.
tests/test_critic_loss_host.py holds it to torch.nn.functional bit for bit; tests/test_gpu_critic_loss.py holds the
kernels to it at the kinks."""
import numpy as np

MSE, L1, SMOOTH_L1, HUBER = 0, 1, 2, 3
f32 = np.float32


def loss_term(e, kind, param=0.0):
    e, p = np.asarray(e, f32), f32(param)
    with np.errstate(all='ignore'):
        if kind == MSE:
            return e * e
        z = np.abs(e)
        if kind == HUBER:
            return np.where(z < p, f32(0.5) * e * e, p * (z - f32(0.5) * p)).astype(f32)
        if kind == SMOOTH_L1 and p > 0:
            return np.where(z < p, f32(0.5) * e * e / p, z - f32(0.5) * p).astype(f32)
        return z


def loss_dq(e, kind, param=0.0):
    """d term / d q, unscaled by 1 / B."""
    e, p = np.asarray(e, f32), f32(param)
    with np.errstate(all='ignore'):
        if kind == MSE:
            return f32(2) * e
        if kind == HUBER:
            return np.where(e <= -p, -p, np.where(e >= p, p, e)).astype(f32)
        if kind == SMOOTH_L1 and p > 0:
            return np.where(e <= -p, f32(-1), np.where(e >= p, f32(1), e / p)).astype(f32)
        return (e > 0).astype(f32) - (e < 0).astype(f32)


def rule_of(loss):
    """(kind, float32 param) of a torch loss object: the mapping updaters.critic_loss_rule must make."""
    import torch
    if loss is None or type(loss) is torch.nn.MSELoss:
        return MSE, 0.0
    if type(loss) is torch.nn.L1Loss:
        return L1, 0.0
    if type(loss) is torch.nn.SmoothL1Loss:
        return SMOOTH_L1, float(f32(loss.beta))
    assert type(loss) is torch.nn.HuberLoss
    return HUBER, float(f32(loss.delta))
