"""GPU tests of the off-policy learner's GRADIENT SUMS against float64 autograd of the reference's losses, on the
paths the agents ship by default.  Adam normalises a gradient element by element, so the parameter deltas the other
off-policy tests compare cannot see a uniform scale error or a relative error of about a percent in a gradient;
these tests read the sums each entry leaves for the optimizer (the Adam step only reads them) and hold every tensor
to 1e-5 of its largest element, the statistic slot to the count B and the logged statistics to float64.

- SAC / TD3 / DDPG on the plain fused torsos, on the fp16x2 weight images (csrc/mlpimg.h) and on the float32 passes;
- the images' range: observation columns of mixed magnitude, a small-weight hidden layer, a bounded normaliser,
  and the documented guard (a weight >= 512 turns the sums non-finite);
- D4PG across atom counts, batch sizes and the projection's edges;
- MPO: the ExpectedSARSA critic, the actor step with its dual gradients, floored duals and statistics, and the
  sharded form (tonic_mpo_actor_grad_shard + tonic_mpo_dual_step).

Every test prints the largest relative error it saw (max |got - want| / max |want| over a case's tensors)."""
import ctypes

import numpy as np
import pytest

from test_gpu_offpolicy_torsos import ACTIVATIONS, _grad_sums

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

FLOAT_EPSILON = 1e-8                # updaters/actors.py:6
MPO_STATS = ('policy_mean_loss', 'policy_std_loss', 'kl_mean_loss', 'kl_std_loss', 'alpha_mean_loss',
             'alpha_std_loss', 'temperature_loss', 'temperature')


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


class _Images:
    """tonic_set_tuning('q_images', on) for the duration of a block, the previous value restored after it."""

    def __init__(self, lib, on):
        self.lib, self.on = lib, int(on)

    def __enter__(self):
        from tonic_amd import _lib
        value = ctypes.c_int32(0)
        _lib.check(self.lib.tonic_get_tuning(b'q_images', ctypes.byref(value)), 'tonic_get_tuning')
        self.before = value.value
        _lib.check(self.lib.tonic_set_tuning(b'q_images', self.on), 'tonic_set_tuning')
        return self

    def __exit__(self, *exc):
        from tonic_amd import _lib
        _lib.check(self.lib.tonic_set_tuning(b'q_images', self.before), 'tonic_set_tuning')


# ---------------------------------------------------------------- agents and the float64 restatement

def _agent(kind, O, A, B, sizes=(256, 256), activation='ReLU', atoms=None, S=20, normalizer=None, seed=9,
           **mpo):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    act = ACTIVATIONS[activation]
    if kind == 'sac':
        head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                            distribution=tt.models.SquashedMultivariateNormalDiag)
    elif kind == 'mpo':
        head = tt.models.GaussianPolicyHead()
    else:
        head = tt.models.DeterministicPolicyHead()
    critic_head = tt.models.DistributionalValueHead(*atoms) if kind == 'd4pg' else tt.models.ValueHead()
    container = tt.models.ActorTwinCriticWithTargets if kind in ('sac', 'td3') else tt.models.ActorCriticWithTargets
    model = container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, act), head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                                head=critic_head),
        observation_normalizer=normalizer if normalizer is not None else tt.normalizers.MeanStd())
    replay = tonic_amd.replays.Buffer(size=1000, batch_iterations=1, batch_size=B)
    if kind == 'mpo':
        agent = tt.agents.MPO(model=model, replay=replay,
                              actor_updater=tt.updaters.MaximumAPosterioriPolicyOptimization(num_samples=S, **mpo),
                              critic_updater=tt.updaters.ExpectedSARSA(num_samples=S))
    else:
        agent = dict(sac=tt.agents.SAC, td3=tt.agents.TD3, ddpg=tt.agents.DDPG,
                     d4pg=tt.agents.D4PG)[kind](model=model, replay=replay)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=seed)
    assert agent.critic_updater.stock is False and agent.actor_updater.stock is False
    return agent


def _set_normalizer(agent, mean, std):
    norm = agent.model.observation_normalizer
    with torch.no_grad():
        norm._mean.copy_(torch.as_tensor(np.asarray(mean, np.float32)))
        norm._std.copy_(torch.as_tensor(np.asarray(std, np.float32)))


def _variables(module):
    from tonic_amd.torch.models import network_variables
    return list(network_variables(module))


def _f64(module):
    """float64 CPU leaves of a network's weights / biases (models.network_variables order)."""
    return [p.detach().cpu().double().requires_grad_() for p in _variables(module)]


class Ref:
    """The networks of one model in float64 (the reference's forward passes, models/actors.py, critics.py), with the
    observation normaliser of mean_stds.py on the critics' inputs only: the reference's Actor.initialize hands its
    normaliser to the encoder's `action_space` slot (actors.py:128-129 vs encoders.py:5-8), so its actors read raw
    observations, and so do the kernels.  `record`: a list that receives (W1, first-layer pre-activation, input) of
    every forward with gradients, for the column-wise bound of dW1.  `trace`: a list that receives every torso layer's
    pre-activation of every forward (detached), `scales`: one that receives the Gaussian heads' softplus before its
    clamp: what a test's preconditions on its inputs read.  `agent`: anything with `.model.observation_normalizer`."""

    def __init__(self, agent, kind, layers, activation):
        self.kind, self.L = kind, layers
        self.act = {'ReLU': torch.relu, 'Tanh': torch.tanh, 'ELU': torch.nn.functional.elu}[activation]
        norm = agent.model.observation_normalizer
        self.mean = norm._mean.detach().cpu().double()
        self.std = norm._std.detach().cpu().double()
        self.clip = norm.clip
        self.record = None
        self.trace = self.scales = None

    def norm(self, obs):
        x = (obs - self.mean) / self.std
        return x if self.clip is None else torch.clamp(x, -self.clip, self.clip)

    def _torso(self, params, x):
        for layer in range(self.L):
            z = torch.nn.functional.linear(x, params[2 * layer], params[2 * layer + 1])
            if layer == 0 and self.record is not None and z.requires_grad:
                z.retain_grad()
                self.record.append((params[0], z, x.detach()))
            if self.trace is not None:
                self.trace.append(z.detach())
            x = self.act(z)
        return x

    def _linear(self, params, h, i):
        return torch.nn.functional.linear(h, params[i], params[i + 1])

    def policy(self, params, obs):
        """(loc or action, scale or None)."""
        h, L = self._torso(params, obs), self.L
        if self.kind in ('sac', 'mpo'):
            loc = self._linear(params, h, 2 * L)
            raw = torch.nn.functional.softplus(self._linear(params, h, 2 * L + 2))
            if self.scales is not None:
                self.scales.append(raw.detach())
            scale = torch.clamp(raw, 1e-4, 1.0)
            return (torch.tanh(loc) if self.kind == 'mpo' else loc), scale
        return torch.tanh(self._linear(params, h, 2 * L)), None

    def critic(self, params, obs, act):
        out = self._linear(params, self._torso(params, torch.cat([self.norm(obs), act], -1)), 2 * self.L)
        return out if self.kind == 'd4pg' else out.squeeze(-1)


def _squashed(loc, scale, noise):
    """SquashedMultivariateNormalDiag.rsample_with_log_prob with the draws given (models/actors.py:11-16)."""
    raw = loc + scale * noise
    a = torch.tanh(raw)
    logp = torch.distributions.Normal(loc, scale).log_prob(raw) - torch.log(1 - a ** 2 + 1e-6)
    return a, logp.sum(-1)


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _check(got, leaves, names, bound=1e-5):
    """Each tensor within `bound` of its largest element; returns the largest relative error of a tensor."""
    worst = 0.0
    for name, g, leaf in zip(names, got, leaves):
        want = leaf.grad.numpy() if hasattr(leaf, 'grad') and leaf.grad is not None else np.asarray(leaf)
        g = g.double().cpu().numpy() if torch.is_tensor(g) else np.asarray(g, np.float64)
        if bound is not None:
            scale = max(np.abs(want).max(), 1e-30)
            np.testing.assert_allclose(g, want, rtol=0, atol=bound * scale, err_msg=name)
        worst = max(worst, _rel(g, want))
    return worst


def _network_error(got, leaves):
    """max |got - want| / max |want| over a network's whole gradient block: the yardstick measure of
    test_fp16x2_layer_one_with_observations_of_mixed_magnitude."""
    diff = max(float((g.double().cpu() - leaf.grad).abs().max()) for g, leaf in zip(got, leaves))
    return diff / max(max(float(leaf.grad.abs().max()) for leaf in leaves), 1e-30)


def _check_stat(got, want, terms, name):
    """A logged statistic (a batch sum or mean) within rtol 1e-5 of float64.  A sum of terms of both signs can cancel
    far below its terms, where float32 summation is only as exact as the terms are large, so the bound also admits
    1e-5 of the mean absolute term."""
    want, scale = float(want), float(torch.as_tensor(terms).abs().mean()) if terms is not None else 0.0
    assert abs(float(got) - want) <= 1e-5 * max(abs(want), scale), (name, float(got), want, scale)
    return abs(float(got) - want) / max(abs(want), 1e-30)


def _stats(updater):
    torch.cuda.synchronize()
    return updater.grad_sums[updater.count:].cpu().numpy()


def _batch(rng, B, O, A):
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32))              # noqa: E731
    return dict(observations=f32(rng.normal(size=(B, O))), actions=f32(rng.uniform(-1, 1, (B, A))),
                next_observations=f32(rng.normal(size=(B, O))), rewards=f32(rng.normal(size=B) * 2),
                discounts=f32(np.full(B, 0.99) * (rng.uniform(size=B) > 0.1)))


# ---------------------------------------------------------------- 1 + 2. SAC / TD3 / DDPG

Q_HYPER = dict(entropy_coeff=0.2, noise_scale=0.2, noise_clip=0.5)     # the updaters' defaults (critics.py, actors.py)


def _q_hyper(agent, kind):
    """What the float64 restatement reads of the updaters: SAC's coefficient, TD3's target-action noise."""
    critic_u, actor_u = agent.critic_updater, agent.actor_updater
    hyper = {}
    if kind == 'sac':
        hyper.update(entropy_coeff=critic_u.entropy_coeff, actor_entropy_coeff=actor_u.entropy_coeff)
    if kind == 'td3':
        noise = critic_u.target_action_noise
        hyper.update(noise_scale=noise.scale, noise_clip=noise.clip)
    return hyper


def _q_leaves(model, kind):
    """float64 leaves of a model's networks: dict(actor, target_actor, online = [critics], frozen = [targets])."""
    twin = kind in ('sac', 'td3')
    critics = [model.critic_1, model.critic_2] if twin else [model.critic]
    targets = [model.target_critic_1, model.target_critic_2] if twin else [model.target_critic]
    return dict(actor=_f64(model.actor), target_actor=_f64(model.target_actor),
                online=[_f64(c) for c in critics], frozen=[_f64(c) for c in targets])


def _q_critic_reference(ref, kind, nets, d, eps, hyper):
    """The critic step's loss in float64 (critics.py), backward into nets['online']: dict(loss, qs, returns, targets
    — each target critic's value of (s', a') — and for TD3 loc / noise, the target action's terms before their
    clamps)."""
    out = {}
    with torch.no_grad():
        if kind == 'sac':                                                   # critics.py:202-235
            loc, scale = ref.policy(nets['actor'], d['next_observations'])
            a, logp = _squashed(loc, scale, eps.to(loc.dtype))
            out['targets'] = [ref.critic(p, d['next_observations'], a) for p in nets['frozen']]
            nxt = torch.min(*out['targets']) - hyper['entropy_coeff'] * logp
        else:
            a = ref.policy(nets['target_actor'], d['next_observations'])[0]
            if kind == 'td3':                                               # critics.py:125-134, :156-182
                out['loc'], out['noise'] = a, hyper['noise_scale'] * eps.to(a.dtype)
                a = torch.clamp(a + torch.clamp(out['noise'], -hyper['noise_clip'], hyper['noise_clip']), -1, 1)
                out['targets'] = [ref.critic(p, d['next_observations'], a) for p in nets['frozen']]
                nxt = torch.min(*out['targets'])
            else:                                                           # critics.py:68-86 (DDPG)
                nxt = ref.critic(nets['frozen'][0], d['next_observations'], a)
                out['targets'] = [nxt]
        returns = d['rewards'] + d['discounts'] * nxt
    qs = [ref.critic(p, d['observations'], d['actions']) for p in nets['online']]
    loss = sum(((q - returns) ** 2).mean() for q in qs)
    loss.backward()
    out.update(loss=loss.detach(), qs=[q.detach() for q in qs], returns=returns)
    return out


def _q_actor_reference(ref, kind, actor, online, d, eps_actor, hyper):
    """The actor step's loss in float64 (actors.py) through the critics `online`, backward into `actor`:
    dict(terms — the rows' losses —, qs — each critic's value of (s, actor(s)))."""
    if kind == 'sac':                                                       # actors.py:238-267
        loc, scale = ref.policy(actor, d['observations'])
        a, logp = _squashed(loc, scale, eps_actor.to(loc.dtype))
        qs = [ref.critic(p, d['observations'], a) for p in online]
        terms = hyper.get('actor_entropy_coeff', hyper['entropy_coeff']) * logp - torch.min(*qs)
    else:                                                                   # actors.py:170-189 (critic_1)
        qs = [ref.critic(online[0], d['observations'], ref.policy(actor, d['observations'])[0])]
        terms = -qs[0]
    terms.mean().backward()
    return dict(terms=terms.detach(), qs=[q.detach() for q in qs])


def _q_steps(agent, kind, batch, eps, eps_actor, ref, bound=1e-5, dw1_columns=False, restore=False):
    """One critic step and one actor step of the HIP entries against float64; returns {'critic': err, 'actor': err}
    (largest relative error of the tensors) and, with bound = None, checks nothing but the statistic slots.
    restore: the online parameters are put back behind the critic step's optimizer, so that the actor step runs
    from the parameters the critic step ran from (else: through the critics the critic step has just moved).
    Also returned: grads / actor_grads, the two gradient-sum blocks as left for the optimizer, and critic_stats /
    actor_stats, their eight statistic slots."""
    m, B = agent.model, batch['observations'].shape[0]
    critic_u, actor_u = agent.critic_updater, agent.actor_updater
    twin = kind in ('sac', 'td3')
    critics = [m.critic_1, m.critic_2] if twin else [m.critic]
    hyper = _q_hyper(agent, kind)
    nets = _q_leaves(m, kind)
    actor, online = nets['actor'], nets['online']
    d = {k: v.double() for k, v in batch.items()}
    gpu = {k: v.cuda() for k, v in batch.items()}
    ref.record = [] if dw1_columns else None
    want = _q_critic_reference(ref, kind, nets, d, eps, hyper)
    qs, returns, loss = want['qs'], want['returns'], want['loss']
    records = ref.record
    info = torch.zeros(8, device='cuda')
    before = m.flat_online.clone() if restore else None
    critic_u.enqueue(gpu, eps.cuda() if eps is not None else None, info)
    stats = _stats(critic_u)
    got = _grad_sums(critics, critic_u.grad_sums, B)
    out = dict(grads=critic_u.grad_sums[:critic_u.count].cpu().numpy(), critic_stats=stats)
    assert stats[5] == B, stats
    leaves = [leaf for p in online for leaf in p]
    out['critic'] = _check(got, leaves, [f'critic {i}' for i in range(len(got))], bound)
    out['critic_net'] = _network_error(got, leaves)
    if bound is not None:
        sq = sum((q - returns) ** 2 for q in qs)
        _check_stat(stats[0] / B, loss, sq, 'critic loss')
        for i, q in enumerate(qs):
            _check_stat(stats[1 + i] / B, q.mean(), q, f'q{i + 1}')
    if dw1_columns:
        conditions = [((q.abs() + returns.abs()) / (q - returns).abs().clamp_min(1e-300)).numpy() for q in qs]
        out['columns'] = _columns(got, leaves, records, len(online[0]), conditions)
    # the actor step (actors.py), through the critics the critic step has just moved (restore: has left as they were)
    if restore:
        m.flat_online.copy_(before)
    online = [_f64(c) for c in critics]
    ref.record = [] if dw1_columns else None
    terms = _q_actor_reference(ref, kind, actor, online, d, eps_actor, hyper)['terms']
    records = [r for r in ref.record if r[0] is actor[0]] if dw1_columns else None
    ref.record = None
    actor_u.enqueue(gpu['observations'], eps_actor.cuda() if kind == 'sac' else None, info)
    stats = _stats(actor_u)
    assert stats[5] == B, stats
    got = _grad_sums([m.actor], actor_u.grad_sums, B)
    out.update(actor_grads=actor_u.grad_sums[:actor_u.count].cpu().numpy(), actor_stats=stats)
    out['actor'] = _check(got, actor, [f'actor {i}' for i in range(len(actor))], bound)
    out['actor_net'] = _network_error(got, actor)
    if bound is not None:
        _check_stat(stats[0] / B, terms.mean(), terms, 'actor loss')
    if dw1_columns:
        out['columns'] = max(out['columns'], _columns(got, actor, records, len(actor), [np.ones(B)]))
    return out


def _columns(got, leaves, records, per_network, conditions):
    """dW1 column by column: column j within 1e-5 of its own largest entry plus a floor of 2^-16 times the sum of
    its terms' sizes, sum_b c_b |dz1[b]|_inf |x[b, j]| (z.grad holds the 1 / B of the mean already).  Every term
    dz1[b, i] x[b, j] is carried to ~2^-22 of itself by either form (the images' two-term splits drop
    lo.lo <= 2^-22 |a||b|, csrc/mlpimg.h), and so is dz1 by the float32 chain, except where row b's loss gradient is
    itself a difference: a critic's TD error q - r - discount q' is rounded to 2^-24 of |q| + |r + discount q'|,
    which its condition number c_b = (|q| + |returns|) / |q - returns| carries into the whole row (c_b = 1 for an
    actor).  The largest seen is 2^-17.3 of the terms (columns at 1e-3 beside columns at 1e3); a column whose
    inputs had lost their low binary16 term would be off by ~2^-11 of its terms, 2^-11 / sqrt(B) >= 2^-15 of their
    sum when the errors' signs are random (B <= 256), so 2^-16 sits between the two.
    Returns the largest column-wise relative error."""
    worst = 0.0
    for n, (w1, z, x) in enumerate(records):
        g = got[n * per_network].double().cpu().numpy()
        want = leaves[n * per_network].grad.numpy()
        assert leaves[n * per_network] is w1 and want.shape == g.shape
        dz = z.grad.abs().max(1).values.numpy() * conditions[n]             # [B]
        terms = (dz[:, None] * x.abs().numpy()).sum(0)                      # [K]
        for j in range(want.shape[1]):
            col_scale = np.abs(want[:, j]).max()
            err = np.abs(g[:, j] - want[:, j]).max()
            assert err <= 1e-5 * col_scale + 2.0 ** -16 * terms[j], (n, j, err, col_scale, terms[j])
            worst = max(worst, err / max(col_scale, 1e-30))
    return worst


Q_SHAPES = [(17, 6, 256, 256), (111, 8, 256, 1024), (67, 21, 256, 100),        # default, cfg 3, cfg 4 per GPU
            (376, 17, 48, 40), (300, 6, 80, 33), (60, 30, 256, 50), (9, 33, 112, 100)]


@pytest.mark.parametrize('kind', ['sac', 'td3', 'ddpg'])
@pytest.mark.parametrize('O,A,H,B', Q_SHAPES)
def test_q_grads_vs_float64_on_images_and_float32(lib, kind, O, A, H, B):
    """One critic step and one actor step of SAC / TD3 / DDPG on the plain (H, H) ReLU torso with a non-trivial
    MeanStd, from identical parameters, batch and noise: with the fp16x2 weight images (the default) and with the
    float32 passes (q_images = 0).  The fused iteration is bit-identical to these split entries
    (test_fused_iteration_equals_the_split_entry_points), so this pins tonic_q_iteration as well."""
    heads = 2 if kind == 'sac' else 1
    rng = np.random.RandomState(O * 7 + A)
    batch = _batch(rng, B, O, A)
    eps, eps_actor = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32), \
        torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
    mean, std = rng.normal(size=O) * 0.5, np.exp(rng.uniform(-1, 1, O))
    errors = {}
    for images in (1, 0):
        with _Images(lib, images):
            served = lib.tonic_mlp_actor_image_bytes(O, H, A, heads) > 0
            # the images serve every in-range shape: a head of A <= 16 * 4 / heads units over 16 .. 256 units
            if images and heads * ((A + 15) // 16) <= 4:
                assert served, (O, H, A, heads)
            if not images:
                assert not served
            agent = _agent(kind, O, A, B, sizes=(H, H), normalizer=None)
            assert agent.critic_updater.hidden == H
            _set_normalizer(agent, mean, std)
            ref = Ref(agent, kind, 2, 'ReLU')
            out = _q_steps(agent, kind, batch, eps if kind != 'ddpg' else None, eps_actor, ref)
            errors['images' if images and served else 'float32' if not images else 'float32 (no image)'] = \
                (out['critic'], out['actor'])
    print(f'{kind} O={O} A={A} H={H} B={B}: largest relative error (critic, actor)', errors)


# ---- 2. the weight images' range

def _scale_w1_columns(agent, actors, critics):
    """Scales the observation columns of W1 by `actors` in the actor and the target actor, by `critics` in every
    critic and target critic."""
    m = agent.model
    critic_nets = [getattr(m, n) for n in ('critic_1', 'critic_2', 'target_critic_1', 'target_critic_2')]
    with torch.no_grad():
        for nets, factors in (([m.actor, m.target_actor], actors), (critic_nets, critics)):
            f = torch.as_tensor(np.asarray(factors, np.float32), device='cuda')
            for net in nets:
                w1 = _variables(net)[0]
                w1[:, :f.numel()] *= f


@pytest.mark.parametrize('kind', ['sac', 'td3'])
@pytest.mark.parametrize('case', ['mixed', 'mixed_conditioned', 'outlier', 'small_w2', 'clip5'])
def test_image_range_vs_float64(lib, kind, case):
    """The fp16x2 images against the float32 passes as a yardstick (the rule of
    test_fp16x2_layer_one_with_observations_of_mixed_magnitude): the image form's error (max |got - want| / max |want|
    over a network's gradient block) at most 4 x the float32 form's + 1e-8 (see the call site); in the conditioned cases both forms also within 1e-5 of float64.
    mixed: normalised observation columns spanning 1e-3 .. 1e3, raw ones (the actors' inputs) as well (W1 as
    initialised, and conditioned: W1's columns scaled by the inverse input scales, where dW1 is also checked column by
    column — as initialised, the 1e3 columns dominate every pre-activation and a column's float32 error reaches
    2^-16 of its terms); outlier: one sample with one column at 1e4 of
    the rest, clip=None; small_w2: the second hidden layer at max |w| = 1e-3 (the images' absolute grid is 2^-32);
    clip5: MeanStd(clip=5) with inputs on the clip."""
    import tonic_amd.torch as tt
    O, A, H, B = 17, 6, 256, 256
    rng = np.random.RandomState(5)
    batch = _batch(rng, B, O, A)
    eps, eps_actor = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32), \
        torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
    exps = np.linspace(-3, 3, O)                                            # log10 of the normalised column scales
    mean, std = np.zeros(O), np.ones(O)
    clip = None
    if case.startswith('mixed'):
        # raw columns at 10^e s (the actors' inputs), normalised ones at 10^e (the critics')
        std = np.exp(rng.uniform(-0.5, 0.5, O))
        for key in ('observations', 'next_observations'):
            batch[key] = batch[key] * torch.as_tensor(10.0 ** exps * std, dtype=torch.float32)
    elif case == 'outlier':
        obs = batch['observations'].numpy().copy()
        obs[7, 3] = 1e4
        batch['observations'] = torch.as_tensor(obs)
    elif case == 'clip5':
        clip = 5
        mean, std = rng.normal(size=O), np.full(O, 0.3)                      # |x| > 5 for a share of the inputs
    conditioned = case in ('mixed_conditioned', 'clip5')
    results = {}
    for images in (1, 0):
        with _Images(lib, images):
            assert (lib.tonic_mlp_actor_image_bytes(O, H, A, 2 if kind == 'sac' else 1) > 0) == bool(images)
            agent = _agent(kind, O, A, B, normalizer=tt.normalizers.MeanStd(clip=clip))
            _set_normalizer(agent, mean, std)
            if case == 'mixed_conditioned':
                _scale_w1_columns(agent, 10.0 ** -exps / std, 10.0 ** -exps)
            if case == 'small_w2':
                m = agent.model
                with torch.no_grad():
                    for net in (m.actor, m.target_actor, m.critic_1, m.critic_2, m.target_critic_1,
                                m.target_critic_2):
                        w2 = _variables(net)[2]
                        w2 *= 1e-3 / w2.abs().max()
            ref = Ref(agent, kind, 2, 'ReLU')
            out = _q_steps(agent, kind, batch, eps, eps_actor, ref, bound=1e-5 if conditioned else None,
                           dw1_columns=case == 'mixed_conditioned')
            results[images] = out
    if clip is not None:
        x = (batch['observations'].numpy() - mean) / std
        assert (np.abs(x) > clip).mean() > 0.05
    for part in ('critic', 'actor'):
        net = results[1][part + '_net'], results[0][part + '_net']
        # 4x, not the 2x of the PPO test: every image product carries ~22 significant bits (the dropped lo.lo term,
        # <= 2^-22 |a||b|, csrc/mlpimg.h) against float32's 24, and the off-policy gradients hold up to 2.8x the
        # float32 form's error (TD3, max |w2| = 1e-3: 2.0e-7 against 7.4e-8), each well inside the 1e-5 bound
        assert net[0] <= 4 * net[1] + 1e-8, (part, net)
    print(f'{kind} {case}: largest relative error (images / float32): critic '
          f'{results[1]["critic"]:.2e} / {results[0]["critic"]:.2e}, actor {results[1]["actor"]:.2e} / '
          f'{results[0]["actor"]:.2e}' + (f', dW1 columns {results[1]["columns"]:.2e} / {results[0]["columns"]:.2e}'
                                           if 'columns' in results[1] else ''))


def test_a_weight_beyond_the_image_range_is_loud(lib):
    """csrc/mlpimg.h: a weight >= 512 has no image; it must turn the gradient sums non-finite, not finite and wrong.
    The float32 passes take the same network and stay finite."""
    O, A, H, B = 17, 6, 256, 64
    rng = np.random.RandomState(2)
    batch = _batch(rng, B, O, A)
    eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32).cuda()
    finite = {}
    for images in (1, 0):
        with _Images(lib, images):
            agent = _agent('sac', O, A, B)
            with torch.no_grad():
                _variables(agent.model.critic_1)[2][3, 5] = 600.0
            agent.critic_updater.enqueue({k: v.cuda() for k, v in batch.items()}, eps, torch.zeros(8, device='cuda'))
            torch.cuda.synchronize()
            finite[images] = bool(torch.isfinite(agent.critic_updater.grad_sums[:agent.critic_updater.count]).all())
    assert finite == {1: False, 0: True}, finite


# ---------------------------------------------------------------- 3. D4PG

def _d4pg_returns(rng, B, NA, returns):
    """(atoms, rewards, discounts) of test_d4pg_grads_vs_float64's two generators."""
    if returns == 'edges':
        atoms = (-10.0, 10.0, NA)
        pushed = rng.uniform(size=B) < 0.8
        pushed[0] = True
        rewards = rng.choice([-1.0, 1.0], B) * rng.uniform(25, 40, B) * pushed + rng.normal(size=B)
        discounts = np.where(rng.uniform(size=B) < 0.25, 0.0, 0.99)
    else:
        atoms = ((1 - NA) / 2, (NA - 1) / 2, NA)
        rewards = rng.randint(-3, 4, B).astype(np.float64)
        discounts = np.ones(B)
    return atoms, rewards, discounts


def _d4pg_critic_reference(ref, target_actor, frozen, online, d, values):
    """critics.py:100-122 in float64, backward into `online`: dict(terms, ret, delta)."""
    with torch.no_grad():
        a = ref.policy(target_actor, d['next_observations'])[0]
        p_next = torch.softmax(ref.critic(frozen, d['next_observations'], a), -1)
        ret = d['rewards'][:, None] + d['discounts'][:, None] * values[None]
        above = (torch.cat([values[1:], values[:1]]) - values)[None, :, None]
        below = (values - torch.cat([values[-1:], values[:-1]]))[None, :, None]
        delta = torch.clamp(ret, values[0], values[-1])[:, None] - values[None, :, None]
        up = (delta >= 0).double()
        hat = (up * delta / above) - ((1 - up) * delta / below)
        target = (torch.clamp(1 - hat, 0, 1) * p_next[:, None]).sum(2)
    terms = -(target * torch.log_softmax(ref.critic(online, d['observations'], d['actions']), -1)).sum(-1)
    terms.mean().backward()
    return dict(terms=terms.detach(), ret=ret, delta=delta)


def _d4pg_actor_reference(ref, actor, online, d, values):
    """actors.py:203-224 in float64, backward into `actor`: (the rows' losses, the rows' sum_i p_i |z_i| — the size of
    the terms a row's loss is the sum of)."""
    logits = ref.critic(online, d['observations'], ref.policy(actor, d['observations'])[0])
    terms = -(torch.softmax(logits, -1) * values).sum(-1)
    terms.mean().backward()
    return terms.detach(), (torch.softmax(logits, -1) * values.abs()).sum(-1).detach()


def _d4pg_steps(agent, batch, ref, restore=False):
    """One critic step and one actor step of the D4PG entries against float64 (see _q_steps): the references, the
    gradient blocks and statistic slots as left for the optimizer, and the largest relative errors."""
    m, B = agent.model, batch['observations'].shape[0]
    critic_u, actor_u = agent.critic_updater, agent.actor_updater
    values = m.target_critic.head.values.double()
    target_actor, frozen, online, actor = _f64(m.target_actor), _f64(m.target_critic), _f64(m.critic), _f64(m.actor)
    d = {k: v.double() for k, v in batch.items()}
    out = _d4pg_critic_reference(ref, target_actor, frozen, online, d, values)
    terms = out['terms']
    info = torch.zeros(8, device='cuda')
    gpu = {k: v.cuda() for k, v in batch.items()}
    before = m.flat_online.clone() if restore else None
    critic_u.enqueue(gpu, None, info)
    stats = _stats(critic_u)
    assert stats[5] == B, stats
    out.update(grads=critic_u.grad_sums[:critic_u.count].cpu().numpy(), critic_stats=stats)
    out['critic'] = _check(_grad_sums([m.critic], critic_u.grad_sums, B), online,
                           [f'critic {i}' for i in range(len(online))])
    _check_stat(stats[0] / B, terms.mean(), terms, 'critic loss')
    if restore:
        m.flat_online.copy_(before)
    online = _f64(m.critic)                                                 # actors.py:203-224, the moved critic
    terms = _d4pg_actor_reference(ref, actor, online, d, agent.actor_updater.values.double().cpu())[0]
    actor_u.enqueue(gpu['observations'], None, info)
    stats = _stats(actor_u)
    assert stats[5] == B, stats
    out.update(actor_grads=actor_u.grad_sums[:actor_u.count].cpu().numpy(), actor_stats=stats)
    out['actor'] = _check(_grad_sums([m.actor], actor_u.grad_sums, B), actor, [f'actor {i}' for i in range(len(actor))])
    _check_stat(stats[0] / B, terms.mean(), terms, 'actor loss')
    return out


@pytest.mark.parametrize('torso', ['plain', 'uneven'])
@pytest.mark.parametrize('NA', [2, 16, 17, 51, 64])
@pytest.mark.parametrize('B', [1, 37, 256])
@pytest.mark.parametrize('returns', ['edges', 'on_atoms'])
def test_d4pg_grads_vs_float64(lib, torso, NA, B, returns):
    """tonic_distributional_q_grad, its loss statistic and tonic_distributional_actor_grad against float64 of
    critics.py:89-122 / actors.py:203-224.  edges: support [-10, 10], most returns past vmin or vmax, a share of
    discounts exactly 0; on_atoms: a support of (half-)integers 1 apart, integer rewards and discount 1, so that every
    return lands exactly on an atom or beyond the support (the projection's delta >= 0 branch).  The float64 side
    projects onto the head's float32 support."""
    O, A = 17, 6
    sizes = (256, 256) if torso == 'plain' else (96, 64)
    rng = np.random.RandomState(NA * 31 + B)
    atoms, rewards, discounts = _d4pg_returns(rng, B, NA, returns)
    agent = _agent('d4pg', O, A, B, sizes=sizes, atoms=atoms)
    assert (agent.critic_updater.hidden == 256) == (torso == 'plain')
    values = agent.model.target_critic.head.values.double()
    if returns == 'on_atoms':
        assert np.array_equal(values.numpy(), np.arange(NA) + (1 - NA) / 2)
    _set_normalizer(agent, rng.normal(size=O) * 0.3, np.exp(rng.uniform(-0.5, 0.5, O)))
    batch = _batch(rng, B, O, A)
    batch['rewards'] = torch.as_tensor(rewards, dtype=torch.float32)
    batch['discounts'] = torch.as_tensor(discounts, dtype=torch.float32)
    ret = batch['rewards'].double()[:, None] + batch['discounts'].double()[:, None] * values[None]
    if returns == 'edges':
        assert (ret[:, 0] < values[0]).any() or B == 1
        assert ((ret < values[0]) | (ret > values[-1])).double().mean() > 0.5
    out = _d4pg_steps(agent, batch, Ref(agent, 'd4pg', len(sizes), 'ReLU'))
    if returns == 'on_atoms':
        assert (out['delta'] == 0).any()
    print(f'd4pg {torso} NA={NA} B={B} {returns}: largest relative error critic {out["critic"]:.2e} '
          f'actor {out["actor"]:.2e}')


# ---------------------------------------------------------------- 4. MPO

MPO_TORSOS = {'plain': ((256, 256), 'ReLU'), 'elu3': ((64, 48, 40), 'ELU')}


def _sarsa_reference(ref, target_actor, frozen, online, d, eps, S):
    """critics.py:238-282 at S samples in float64, backward into `online`: (the rows' squared errors, q)."""
    B, A = d['observations'].shape[0], eps.shape[-1]
    with torch.no_grad():
        loc, scale = ref.policy(target_actor, d['next_observations'])
        a = (loc[None] + scale[None] * eps.to(loc.dtype).view(S, B, A)).reshape(S * B, A)
        nxt = ref.critic(frozen, d['next_observations'].repeat(S, 1), a).view(S, B).mean(0)
        returns = d['rewards'] + d['discounts'] * nxt
    q = ref.critic(online, d['observations'], d['actions'])
    sq = (q - returns) ** 2
    sq.mean().backward()
    return sq.detach(), q.detach()


def _sarsa_step(agent, batch, eps, ref, S):
    """tonic_expected_sarsa_grad against float64: dict(critic, the largest relative error; grads, critic_stats)."""
    m, u, B = agent.model, agent.critic_updater, batch['observations'].shape[0]
    target_actor, frozen, online = _f64(m.target_actor), _f64(m.target_critic), _f64(m.critic)
    sq, q = _sarsa_reference(ref, target_actor, frozen, online, {k: v.double() for k, v in batch.items()}, eps, S)
    u.enqueue({k: v.cuda() for k, v in batch.items()}, eps.cuda(), torch.zeros(8, device='cuda'))
    stats = _stats(u)
    assert stats[5] == B, stats
    err = _check(_grad_sums([m.critic], u.grad_sums, B), online, [f'critic {i}' for i in range(len(online))])
    _check_stat(stats[0] / B, sq.mean(), sq, 'loss')
    _check_stat(stats[1] / B, q.mean(), q, 'q')
    return dict(critic=err, grads=u.grad_sums[:u.count].cpu().numpy(), critic_stats=stats)


@pytest.mark.parametrize('torso', ['plain', 'elu3'])
@pytest.mark.parametrize('S', [1, 20, 64])
def test_expected_sarsa_grads_vs_float64(lib, torso, S):
    """tonic_expected_sarsa_grad and its statistics against float64 of critics.py:238-282 at S samples."""
    O, A, B = 17, 6, 256
    sizes, activation = MPO_TORSOS[torso]
    rng = np.random.RandomState(S)
    agent = _agent('mpo', O, A, B, sizes=sizes, activation=activation, S=S)
    _set_normalizer(agent, rng.normal(size=O) * 0.3, np.exp(rng.uniform(-0.5, 0.5, O)))
    batch = _batch(rng, B, O, A)
    eps = torch.as_tensor(rng.normal(size=(S * B, A)), dtype=torch.float32)
    err = _sarsa_step(agent, batch, eps, Ref(agent, 'mpo', len(sizes), activation), S)['critic']
    print(f'mpo critic {torso} S={S}: largest relative error {err:.2e}')


def _mpo_reference(ref, actor, target_actor, frozen, obs, eps, duals, floor, u, S, penalization):
    """actors.py:318-464 with per_dim_constraining=True in float64: returns (loss, dual leaves, stats, actions)."""
    B, A = obs.shape[0], eps.shape[-1]
    with torch.no_grad():
        loc_t, scale_t = ref.policy(target_actor, obs)
        actions = loc_t[None] + scale_t[None] * eps.view(S, B, A)
        values = ref.critic(frozen, obs.repeat(S, 1), actions.reshape(S * B, A)).view(S, B)
    floored = torch.maximum(torch.as_tensor(duals, dtype=torch.float64),
                            torch.tensor(float(np.float32(floor)), dtype=torch.float64))
    log_t = floored[:1].clone().requires_grad_()
    log_am = floored[1:1 + A].clone().requires_grad_()
    log_as = floored[1 + A:1 + 2 * A].clone().requires_grad_()
    log_p = floored[1 + 2 * A:].clone().requires_grad_()
    softplus = torch.nn.functional.softplus

    scales = []          # the size of the temperature losses' terms: T (|epsilon| + mean |LSE| + log S)

    def weights_and_loss(q, epsilon, temperature):
        tempered = q.detach() / temperature
        weights = torch.softmax(tempered, 0).detach()
        lse = torch.logsumexp(tempered, 0)
        scales.append(float(temperature) * (abs(epsilon) + float(lse.abs().mean()) + np.log(q.shape[0])))
        return weights, temperature * (epsilon + lse.mean() - np.log(q.shape[0]))

    loc, scale = ref.policy(actor, obs)
    temperature = softplus(log_t) + FLOAT_EPSILON
    alpha_mean, alpha_std = softplus(log_am) + FLOAT_EPSILON, softplus(log_as) + FLOAT_EPSILON
    weights, temperature_loss = weights_and_loss(values, u.epsilon, temperature)
    penalty_temperature = softplus(log_p) + FLOAT_EPSILON
    if penalization:
        costs = -torch.norm(actions - torch.clamp(actions, -1, 1), dim=-1)
        pw, pl = weights_and_loss(costs, u.epsilon_penalty, penalty_temperature)
        weights = weights + pw
        temperature_loss = temperature_loss + pl
    normal = torch.distributions.Normal
    fixed_std, fixed_mean = normal(loc, scale_t), normal(loc_t, scale)
    policy_mean_loss = -((fixed_std.log_prob(actions).sum(-1) * weights).sum(0)).mean()
    policy_std_loss = -((fixed_mean.log_prob(actions).sum(-1) * weights).sum(0)).mean()
    target = normal(loc_t, scale_t)
    kl_mean = torch.distributions.kl.kl_divergence(target, fixed_std).mean(0)
    kl_std = torch.distributions.kl.kl_divergence(target, fixed_mean).mean(0)
    kl_mean_loss, alpha_mean_loss = (alpha_mean.detach() * kl_mean).sum(), \
        (alpha_mean * (u.epsilon_mean - kl_mean.detach())).sum()
    kl_std_loss, alpha_std_loss = (alpha_std.detach() * kl_std).sum(), \
        (alpha_std * (u.epsilon_std - kl_std.detach())).sum()
    loss = policy_mean_loss + policy_std_loss + kl_mean_loss + kl_std_loss + alpha_mean_loss + alpha_std_loss + \
        temperature_loss
    loss.backward()
    stats = [policy_mean_loss, policy_std_loss, kl_mean_loss, kl_std_loss, alpha_mean_loss, alpha_std_loss,
             temperature_loss, temperature[0]]
    stats = np.concatenate([np.array([float(s) for s in stats]), alpha_mean.detach().numpy(),
                            alpha_std.detach().numpy(), penalty_temperature.detach().numpy()])
    actor_loss = float(policy_mean_loss + policy_std_loss + kl_mean_loss + kl_std_loss)
    tempering = float(values.abs().max() / temperature)         # max |Q| / T
    return (log_t, log_am, log_as, log_p), stats, actor_loss, floored.numpy(), actions, sum(scales), tempering


def _mpo_duals(A, log_temperature=-5.0):
    """[log T | log alpha_mean | log alpha_std | log penalty T]: duals below the floor, T cold unless given."""
    return np.concatenate([[log_temperature], np.where(np.arange(A) % 2, -25.0, 1.0),
                           np.where(np.arange(A) % 2, 10.0, -30.0), [-20.0]]).astype(np.float32)


def _mpo_setup(lib, A, B, torso, penalization, floor, S=20, seed=0):
    """torso: a name of MPO_TORSOS, or (sizes, activation)."""
    O = 17
    sizes, activation = MPO_TORSOS[torso] if isinstance(torso, str) else torso
    rng = np.random.RandomState(seed + A * 13 + B)
    agent = _agent('mpo', O, A, B, sizes=sizes, activation=activation, S=S, action_penalization=penalization,
                   min_log_dual=floor)
    _set_normalizer(agent, rng.normal(size=O) * 0.3, np.exp(rng.uniform(-0.5, 0.5, O)))
    m = agent.model
    with torch.no_grad():
        # the scale head's bias: some dimensions' sigma on the 1e-4 floor, some on the 1 ceiling (both networks)
        for net in (m.actor, m.target_actor):
            b_scale = _variables(net)[-1]
            if A >= 2:
                b_scale[0] = -12.0
                b_scale[1] = 3.0
        # the online actor away from the target: every KL first order
        for p in _variables(m.actor):
            p += torch.as_tensor(rng.normal(size=tuple(p.shape)) * 0.02, dtype=torch.float32, device='cuda')
    u = agent.actor_updater
    duals = _mpo_duals(A)                                          # a cold temperature, duals below the floor
    obs = torch.as_tensor(rng.normal(size=(B, O)), dtype=torch.float32)
    eps = torch.as_tensor(rng.normal(size=(S * B, A)), dtype=torch.float32)
    return agent, u, duals, obs, eps, Ref(agent, 'mpo', len(sizes), activation)


def _mpo_call(lib, agent, u, duals, obs, eps, shard=None):
    """The C entry once (the dual Adam step not run, so that the floored duals can be read); shard = k: the batch
    in k parts through tonic_mpo_actor_grad_shard, column sums added on the host, then tonic_mpo_dual_step."""
    from tonic_amd import _lib
    p, m, A, S = _lib.ptr, agent.model, u.action_size, u.num_samples
    B = obs.shape[0]
    mean, std = u.norm_tensors()
    d_duals = torch.as_tensor(duals).cuda()
    grads = torch.zeros(u.count + 8, device='cuda')
    dual_grads = torch.zeros(2 * A + 2 + 8, device='cuda')
    stats = torch.zeros(9 + 2 * A, device='cuda')
    obs, eps = obs.cuda(), eps.cuda().view(S, B, A)
    if shard is None:
        ws = u._offpolicy_workspace(B)
        _lib.check(lib.tonic_mpo_actor_grad(
            p(m.flat_actor.flat), p(m.flat_target_actor.flat), p(m.flat_target_critics.flat), p(d_duals),
            float(u.min_log_dual), p(mean), p(std), u.norm_clip(), p(obs), p(eps.reshape(S * B, A)), p(grads),
            p(dual_grads), p(stats), B, u.observation_size, u.hidden, A, S, float(u.epsilon), float(u.epsilon_penalty),
            float(u.epsilon_mean), float(u.epsilon_std), int(bool(u.action_penalization)), p(ws), ws.numel(),
            _lib.current_stream()), 'tonic_mpo_actor_grad')
    else:
        columns = torch.zeros(6 + 2 * A, dtype=torch.float64, device='cuda')
        bounds = np.linspace(0, B, shard + 1).astype(int)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            part = torch.zeros(u.count + 8, device='cuda')
            cols = torch.zeros(6 + 2 * A, dtype=torch.float64, device='cuda')
            o, e = obs[lo:hi].contiguous(), eps[:, lo:hi].reshape(S * (hi - lo), A).contiguous()
            ws = u._offpolicy_workspace(hi - lo)
            _lib.check(lib.tonic_mpo_actor_grad_shard(
                p(m.flat_actor.flat), p(m.flat_target_actor.flat), p(m.flat_target_critics.flat), p(d_duals),
                float(u.min_log_dual), p(mean), p(std), u.norm_clip(), p(o), p(e), p(part), p(cols), hi - lo,
                u.observation_size, u.hidden, A, S, int(bool(u.action_penalization)), p(ws), ws.numel(),
                _lib.current_stream()), 'tonic_mpo_actor_grad_shard')
            torch.cuda.synchronize()
            grads[:u.count] += part[:u.count]
            columns += cols
        _lib.check(lib.tonic_mpo_dual_step(
            p(columns), p(d_duals), float(u.min_log_dual), p(dual_grads), p(stats), p(grads[u.count:]), B, B, A, S,
            float(u.epsilon), float(u.epsilon_penalty), float(u.epsilon_mean), float(u.epsilon_std),
            int(bool(u.action_penalization)), _lib.current_stream()), 'tonic_mpo_dual_step')
    torch.cuda.synchronize()
    return (grads.cpu().numpy(), dual_grads.cpu().numpy(), stats.cpu().numpy(), d_duals.cpu().numpy())


def _mpo_compare(agent, u, got, duals, obs, eps, ref, label, bound=None):
    grads, dual_grads, stats, written = got
    m, A, S, B = agent.model, u.action_size, u.num_samples, obs.shape[0]
    actor, target_actor, frozen = _f64(m.actor), _f64(m.target_actor), _f64(m.target_critic)
    penal = bool(u.action_penalization)
    leaves, want_stats, actor_loss, floored, actions, temperature_scale, tempering = _mpo_reference(
        ref, actor, target_actor, frozen, obs.double(), eps.double(), duals, u.min_log_dual, u, S, penal)
    outside = (actions.abs() > 1).double().mean()
    assert 0 < outside < 1, float(outside)                       # the penalty weights are not uniform
    # The E-step weights are softmax_s(Q / T) of float32 Q values: a rounding of Q by 2^-24 |Q| moves them by
    # 2^-24 max |Q| / T relative, 150x more at log T = -5 than at T = 1.  The actor's gradients are held to
    # max(1e-5, 64 x that) of each tensor's largest element (seen: up to 5.2e-5 at A = 1, B = 37, log T = -5, where
    # 16 x would give 2.5e-5; a gradient scaled by 1.001 is still 1e-3 off).
    # (bound given: the caller's, for inputs whose temperature leaves the weights well conditioned)
    bound = max(1e-5, 64 * 2.0 ** -24 * tempering) if bound is None else bound
    err = _check(_grad_sums([m.actor], torch.as_tensor(grads), B), actor, [f'actor {i}' for i in range(len(actor))],
                 bound)
    names = ('log_temperature', 'log_alpha_mean', 'log_alpha_std', 'log_penalty_temperature')
    groups = [np.s_[:1], np.s_[1:1 + A], np.s_[1 + A:1 + 2 * A], np.s_[1 + 2 * A:2 * A + 2]]
    dual_err = 0.0
    for name, leaf, at in zip(names, leaves, groups):
        if name == 'log_penalty_temperature' and not penal:
            assert dual_grads[at][0] == 0.0
            continue
        if name in ('log_temperature', 'log_penalty_temperature'):
            # (epsilon + mean entropy of the weights - log S) sigmoid(log T): a difference of terms up to log S,
            # held to 1e-5 of sigmoid(log T) (|epsilon| + log S) when it cancels below that
            epsilon = u.epsilon if name == 'log_temperature' else u.epsilon_penalty
            want = float(leaf.grad[0])
            scale = max(abs(want), float(torch.sigmoid(leaf.detach()[0])) * (abs(epsilon) + np.log(S)))
            assert abs(float(dual_grads[at][0]) - want) <= 1e-5 * scale, (name, float(dual_grads[at][0]), want)
            dual_err = max(dual_err, abs(float(dual_grads[at][0]) - want) / max(abs(want), 1e-30))
            continue
        dual_err = max(dual_err, _check([torch.as_tensor(dual_grads[at])], [leaf], [name]))
    assert dual_grads[2 * A + 2 + 5] == 1.0, dual_grads[2 * A + 2:]
    # the floored duals written back ahead of the duals' step (the penalty temperature only with penalisation)
    want_written = floored.astype(np.float32)
    if not penal:
        want_written[-1] = duals[-1]
    assert np.array_equal(written, want_written), (written, want_written)
    assert grads[u.count + 5] == B, grads[u.count:]
    _check_stat(grads[u.count] / B, actor_loss, None, 'actor loss slot')
    n = 8 + 2 * A + (1 if penal else 0)
    # (the temperature loss, stat 6, is T (epsilon + mean LSE - log S): a difference of terms of the size of LSE,
    #  held to 1e-5 of T (|epsilon| + mean |LSE| + log S) as well, like any other sum that cancels)
    stat_err = max(_check_stat(stats[i], want_stats[i], torch.tensor([temperature_scale]) if i == 6 else None,
                               f'stat {i}') for i in range(n))
    print(f'mpo actor {label}: largest relative error actor {err:.2e} (bound {bound:.1e}) duals {dual_err:.2e} stats {stat_err:.2e}')
    return err, dual_err, stat_err


@pytest.mark.parametrize('torso', ['plain', 'elu3'])
@pytest.mark.parametrize('A', [1, 6, 64])
@pytest.mark.parametrize('B', [37, 256])
@pytest.mark.parametrize('penalization', [True, False])
def test_mpo_actor_grads_vs_float64(lib, torso, A, B, penalization):
    """tonic_mpo_actor_grad against float64 of actors.py:318-464 (per_dim_constraining=True): the actor's gradient
    sums, d loss / d log-duals, the statistics row, the floored duals it writes back and the statistic slot.  The
    online actor is perturbed away from the target (every KL first order); log T = -5 (the softmax over samples
    saturates); log-duals below min_log_dual; sigma on its 1e-4 floor and its 1 ceiling in some dimensions; sampled
    actions outside [-1, 1]."""
    agent, u, duals, obs, eps, ref = _mpo_setup(lib, A, B, torso, penalization, -18.0)
    got = _mpo_call(lib, agent, u, duals, obs, eps)
    _mpo_compare(agent, u, got, duals, obs, eps, ref, f'{torso} A={A} B={B} penalization={penalization}')


@pytest.mark.parametrize('torso', ['plain', 'elu3'])
def test_mpo_actor_grads_with_a_raised_dual_floor(lib, torso):
    """min_log_dual = -3: the cold temperature and most duals sit on the floor, read through it and written back."""
    agent, u, duals, obs, eps, ref = _mpo_setup(lib, 6, 100, torso, True, -3.0)
    got = _mpo_call(lib, agent, u, duals, obs, eps)
    assert (got[3] == np.float32(-3.0)).sum() >= 4
    _mpo_compare(agent, u, got, duals, obs, eps, ref, f'{torso} floor -3')


@pytest.mark.parametrize('torso', ['plain', 'elu3'])
@pytest.mark.parametrize('penalization', [True, False])
def test_mpo_sharded_step_equals_the_single_call(lib, torso, penalization):
    """The batch in two halves through tonic_mpo_actor_grad_shard, column sums added on the host, then
    tonic_mpo_dual_step: dual gradients, statistics, slots and written duals equal the single call's to the rounding
    of the float64 column sums (their order of summation differs), and match float64."""
    agent, u, duals, obs, eps, ref = _mpo_setup(lib, 6, 256, torso, penalization, -18.0)
    single = _mpo_call(lib, agent, u, duals, obs, eps)
    sharded = _mpo_call(lib, agent, u, duals, obs, eps, shard=2)
    A = u.action_size
    np.testing.assert_allclose(sharded[1][:2 * A + 2], single[1][:2 * A + 2], rtol=1e-6, atol=0)
    np.testing.assert_allclose(sharded[2], single[2], rtol=1e-6, atol=0)
    assert np.array_equal(sharded[3], single[3])
    assert sharded[0][u.count + 5] == single[0][u.count + 5] == obs.shape[0]
    _mpo_compare(agent, u, sharded, duals, obs, eps, ref, f'{torso} sharded penalization={penalization}')
