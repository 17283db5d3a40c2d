"""Float64 NumPy statement of TRPO's actor mathematics (helper of test_trpo_fisher_host.py and
test_gpu_trpo_hip.py, no test itself).

Actor: hidden layers h_l = act(h_{l-1} W_l^T + b_l) from h_0 = x, head mu = tanh(h_L W_mu^T + b_mu),
sigma_a = clamp(softplus(s_a) + 1e-8, 1e-4, 1) with s the [1, A] log_scale.  Parameters travel as ONE flat
vector in parameters() order: per layer W [size, fan_in] then b [size], then log_scale [A], W_mu [A, last],
b_mu [A].

    L(theta)  = -mean_n(exp(logp(a) - logp_old) * adv) - entropy_coeff * mean_{n,A}(entropy)
    KL(theta) = mean_{n,A}(log(sigma_o / sigma) + (sigma^2 + (mu - mu_o)^2) / (2 sigma_o^2) - 1/2)

and, at (mu_o, sigma_o) = the network's own output, the Gauss-Newton product F v = J^T M J v of KL.  Every
function returns SUMS over the rows (n * L, n * A * KL, ...), the form the kernels return.
"""
import numpy as np

FLOAT_EPSILON = 1e-8
SCALE_MIN, SCALE_MAX = 1e-4, 1.0
LOG_SQRT_2PI = 0.5 * np.log(2 * np.pi)


def layout(O, A, sizes):
    """[(name, shape, offset)] of the flat vector and its length."""
    out, at, fan_in = [], 0, O
    for l, size in enumerate(sizes):
        out.append((f'W{l}', (size, fan_in), at)); at += size * fan_in
        out.append((f'b{l}', (size,), at)); at += size
        fan_in = size
    out.append(('log_scale', (A,), at)); at += A
    out.append(('W_mu', (A, fan_in), at)); at += A * fan_in
    out.append(('b_mu', (A,), at)); at += A
    return out, at


def unpack(theta, O, A, sizes):
    theta = np.asarray(theta, np.float64)
    return {name: theta[at:at + int(np.prod(shape))].reshape(shape) for name, shape, at in layout(O, A, sizes)[0]}


def pack(tensors, O, A, sizes):
    slots, count = layout(O, A, sizes)
    flat = np.zeros(count, np.float64)
    for name, shape, at in slots:
        flat[at:at + int(np.prod(shape))] = np.asarray(tensors[name], np.float64).reshape(-1)
    return flat


def _act(z, activation):
    return np.tanh(z) if activation == 'tanh' else np.maximum(z, 0.0)


def _act_prime(h, activation):
    """act'(z) from h = act(z)."""
    return 1.0 - h * h if activation == 'tanh' else (h > 0).astype(np.float64)


def scales(log_scale):
    """sigma [A] and d sigma / d log_scale [A]: softplus' = sigmoid inside the clamp, 0 outside."""
    s = np.asarray(log_scale, np.float64)
    raw = np.logaddexp(0.0, s) + FLOAT_EPSILON
    inside = (raw >= SCALE_MIN) & (raw <= SCALE_MAX)
    return np.clip(raw, SCALE_MIN, SCALE_MAX), np.where(inside, 1.0 / (1.0 + np.exp(-s)), 0.0)


def forward(theta, x, O, A, sizes, activation):
    """(hidden activations [h_0 = x, h_1 .. h_L], mu [n, A], sigma [A], d sigma / d log_scale [A])."""
    p = unpack(theta, O, A, sizes)
    hs = [np.asarray(x, np.float64)]
    for l in range(len(sizes)):
        hs.append(_act(hs[-1] @ p[f'W{l}'].T + p[f'b{l}'], activation))
    mu = np.tanh(hs[-1] @ p['W_mu'].T + p['b_mu'])
    sigma, dsigma = scales(p['log_scale'])
    return hs, mu, sigma, dsigma


def _backward(theta, hs, dz_head, dlog_scale, O, A, sizes, activation):
    """Parameter gradient sums from d / d (pre-tanh head output) [n, A] and d / d log_scale [A]."""
    p = unpack(theta, O, A, sizes)
    g = {'log_scale': dlog_scale, 'W_mu': dz_head.T @ hs[-1], 'b_mu': dz_head.sum(0)}
    dh = dz_head @ p['W_mu']
    for l in reversed(range(len(sizes))):
        dz = dh * _act_prime(hs[l + 1], activation)
        g[f'W{l}'] = dz.T @ hs[l]
        g[f'b{l}'] = dz.sum(0)
        dh = dz @ p[f'W{l}']
    return pack(g, O, A, sizes)


def log_probs(mu, sigma, actions):
    return (-(actions - mu) ** 2 / (2 * sigma ** 2) - np.log(sigma) - LOG_SQRT_2PI).sum(-1)


def loss_sum(theta, x, actions, advantages, old_log_probs, entropy_coeff, O, A, sizes, activation):
    """n * L(theta)."""
    _, mu, sigma, _ = forward(theta, x, O, A, sizes, activation)
    ratio = np.exp(log_probs(mu, sigma, np.asarray(actions, np.float64)) - old_log_probs)
    entropy = (0.5 + LOG_SQRT_2PI + np.log(sigma)).mean()
    return -(ratio * advantages).sum() - entropy_coeff * entropy * len(mu)


def loss_grad_sums(theta, x, actions, advantages, old_log_probs, entropy_coeff, O, A, sizes, activation):
    """d (n * L) / d theta [P]."""
    hs, mu, sigma, dsigma = forward(theta, x, O, A, sizes, activation)
    actions = np.asarray(actions, np.float64)
    ratio = np.exp(log_probs(mu, sigma, actions) - old_log_probs)
    g = -(ratio * advantages)[:, None]                              # d / d logp per row
    dif = actions - mu
    dz_head = g * dif / sigma ** 2 * (1.0 - mu * mu)
    dsig = (g * (dif ** 2 / sigma ** 3 - 1.0 / sigma)).sum(0) - entropy_coeff * len(mu) / (A * sigma)
    return _backward(theta, hs, dz_head, dsig * dsigma, O, A, sizes, activation)


def kl_sum(theta, x, mu_o, sigma_o, O, A, sizes, activation):
    """n * A * KL(theta)."""
    _, mu, sigma, _ = forward(theta, x, O, A, sizes, activation)
    return (np.log(sigma_o / sigma) + (sigma ** 2 + (mu - mu_o) ** 2) / (2 * sigma_o ** 2) - 0.5).sum()


def fisher_vector_sums(theta, x, v, O, A, sizes, activation):
    """sum over the rows of J^T M J v [P] (divide by n * A for the Hessian of the mean KL)."""
    p, pv = unpack(theta, O, A, sizes), unpack(v, O, A, sizes)
    hs, mu, sigma, dsigma = forward(theta, x, O, A, sizes, activation)
    tangent = np.zeros_like(hs[0])
    for l in range(len(sizes)):                                     # tangent pass J v
        tangent = _act_prime(hs[l + 1], activation) * (tangent @ p[f'W{l}'].T + hs[l] @ pv[f'W{l}'].T + pv[f'b{l}'])
    mu_dot = (1.0 - mu * mu) * (tangent @ p['W_mu'].T + hs[-1] @ pv['W_mu'].T + pv['b_mu'])
    sigma_dot = dsigma * pv['log_scale']
    c_mu = mu_dot / sigma ** 2                                      # the metric M, per element
    c_sigma = 2.0 * sigma_dot / sigma ** 2
    return _backward(theta, hs, c_mu * (1.0 - mu * mu), dsigma * c_sigma * len(mu), O, A, sizes, activation)
