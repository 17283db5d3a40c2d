"""Prioritized replay on the GPU, above the tree (tests/test_gpu_priority_tree.py holds the tree itself):

1. the weighted critic steps of D4PG and TD4 — NULL / NULL bit-identical to the unweighted entries; gradient
   sums, the weighted loss statistic and the rows' unweighted losses against float64 autograd of the weighted loss
   (the Ref machinery of tests/test_gpu_offpolicy_grads.py, tests/td4_ref.py and their bounds);
2. whole update calls of D4PG and TD4 on a small PrioritizedBuffer: the captured graph against a step-by-step host
   loop of the four entries bit for bit, the indices of every iteration against the NumPy tree fed with the read-back
   losses, a second call that replays the graph and follows the moved priorities;
3. the refusal of an agent that is not served, and a uniform-Buffer D4PG update held to the bits the parent commit
   gave (tests/golden/uniform_d4pg_update_bits.json, recorded there by `uniform_update_digest` below).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import prioritized_ref
import td4_ref
from test_gpu_offpolicy_grads import Ref, _batch, _check, _check_stat, _f64, _set_normalizer
from test_gpu_offpolicy_torsos import _grad_sums
from test_gpu_td4 import _agent, _search, _spread_targets

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

O, A = 17, 6
SUPPORT = (-10.0, 10.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'uniform_d4pg_update_bits.json')


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def _weights(rng, B):
    """Importance weights spanning 1e-3 .. 1, both ends present."""
    w = np.exp(rng.uniform(np.log(1e-3), 0.0, B))
    w[0], w[-1] = 1.0, 1e-3
    return torch.as_tensor(w, dtype=torch.float32)


def _enqueue(agent, batch, eps, weights=None, sample_losses=None):
    """One call of the critic updater's entry on fresh sums: (sums and statistics, a clone), the parameters and the
    optimizer's state put back behind the step that follows it."""
    updater, model = agent.critic_updater, agent.model
    keep = [t.clone() for t in (model.flat_online, updater.exp_avg, updater.exp_avg_sq, updater.state)]
    more = {} if weights is None and sample_losses is None else dict(weights=weights, sample_losses=sample_losses)
    updater.enqueue({k: v.cuda() for k, v in batch.items()}, None if eps is None else eps.cuda(),
                    torch.zeros(8, device='cuda'), **more)
    torch.cuda.synchronize()
    sums = updater.grad_sums.clone()
    for tensor, kept in zip((model.flat_online, updater.exp_avg, updater.exp_avg_sq, updater.state), keep):
        tensor.copy_(kept)
    return sums


CASES = [pytest.param(B, sizes, NA, id=f'B{B}-{"x".join(map(str, sizes))}-NA{NA}')
         for B in (33, 100) for sizes in ((256, 256), (48, 32)) for NA in (51, 7)]


def _prepared(twin, B, sizes, NA):
    agent = _agent(O, A, sizes, 'ReLU', B, NA, twin=twin)
    assert (agent.critic_updater.hidden == 256) == (sizes == (256, 256))      # (48, 32): the layer-by-layer path
    rng = np.random.RandomState(B * 13 + NA + sizes[0])
    _set_normalizer(agent, rng.normal(size=O) * 0.3, np.exp(rng.uniform(-0.5, 0.5, O)))
    return agent, rng


@pytest.mark.parametrize('B,sizes,NA', CASES)
def test_d4pg_weighted_step(lib, B, sizes, NA):
    agent, rng = _prepared(False, B, sizes, NA)
    m, updater = agent.model, agent.critic_updater
    batch = _batch(rng, B, O, A)
    weights = _weights(rng, B)
    # NULL / NULL: the bits of the unweighted entry (the updater calls the weighted entry only when asked to)
    plain = _enqueue(agent, batch, None)
    p, ws = (lambda t: t.data_ptr()), updater._offpolicy_workspace(B)
    mean, std = updater.norm_tensors()
    gpu = {k: v.cuda() for k, v in batch.items()}

    def raw(entry, *more):
        """The entry by itself (no optimizer step behind it) on sums pre-filled with a pattern: the padding of the weight rows, which no
        entry writes, keeps it."""
        updater.grad_sums.fill_(-12345.0)
        status = getattr(lib, entry)(
            p(m.flat_target_actor.flat), p(m.flat_target_critics.flat), p(updater.flat.flat), p(mean), p(std),
            updater.norm_clip(), p(gpu['observations']), p(gpu['actions']), p(gpu['next_observations']),
            p(gpu['rewards']), p(gpu['discounts']), p(updater.target_values), p(updater.grad_sums), B, O,
            updater.hidden, A, NA, *more, p(ws), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert status == 0, lib.tonic_last_error().decode()
        torch.cuda.synchronize()
        sums = updater.grad_sums.clone().view(torch.int32)
        updater.grad_sums.zero_()
        return sums
    unweighted = raw('tonic_distributional_q_grad')
    assert float((unweighted.view(torch.float32) != -12345.0).float().mean()) > 0.5
    assert torch.equal(raw('tonic_weighted_distributional_q_grad', None, None), unweighted), 'NULL / NULL moved the bits'
    # the losses alone (no weights) leave the sums where they were, too
    losses = torch.full((B + 2,), float('nan'), device='cuda')
    alone = _enqueue(agent, batch, None, sample_losses=losses[1:B + 1])
    assert torch.equal(alone.view(torch.int32), plain.view(torch.int32))
    assert bool(torch.isnan(losses[[0, B + 1]]).all())

    # float64 autograd of mean(w * loss) (critics.py:100-122 with the weight on every row's loss)
    ref = Ref(agent, 'd4pg', len(sizes), 'ReLU')
    values = m.target_critic.head.values.double().cpu()
    target_actor, frozen, online = _f64(m.target_actor), _f64(m.target_critic), _f64(m.critic)
    d = {k: v.double() for k, v in batch.items()}
    with torch.no_grad():
        action = ref.policy(target_actor, d['next_observations'])[0]
        p_next = torch.softmax(ref.critic(frozen, d['next_observations'], action), -1)
        returns = d['rewards'][:, None] + d['discounts'][:, None] * values[None]
        target = td4_ref.categorical(values, torch.log(p_next)).project(returns)
    terms = -(target * torch.log_softmax(ref.critic(online, d['observations'], d['actions']), -1)).sum(-1)
    w64 = weights.double()
    (w64 * terms).mean().backward()
    losses.fill_(float('nan'))
    sums = _enqueue(agent, batch, None, weights=weights.cuda(), sample_losses=losses[1:B + 1])
    stats = sums[updater.count:].cpu().numpy()
    assert stats[5] == B and bool(torch.isnan(losses[[0, B + 1]]).all())
    err = _check(_grad_sums([m.critic], sums, B), online, [f'critic {i}' for i in range(len(online))])
    _check_stat(stats[0] / B, (w64 * terms).detach().mean(), (w64 * terms).detach(), 'weighted loss')
    _check([losses[1:B + 1]], [terms.detach().numpy()], ['sample losses'])
    # the weights alone give the same sums
    again = _enqueue(agent, batch, None, weights=weights.cuda())
    assert torch.equal(again.view(torch.int32), sums.view(torch.int32))
    print(f'd4pg weighted {sizes} B={B} NA={NA}: largest relative error {err:.2e}')


@pytest.mark.parametrize('B,sizes,NA', CASES)
def test_td4_weighted_step(lib, B, sizes, NA):
    agent, rng = _prepared(True, B, sizes, NA)
    m, updater = agent.model, agent.critic_updater
    noise = updater.target_action_noise
    _spread_targets(agent, len(sizes), 'ReLU')
    nets = td4_ref.Networks.of_model(m, len(sizes), 'ReLU')
    batch, eps, d = _search(nets, B, O, A, noise, 100 * B + NA)
    weights = _weights(rng, B)
    plain = _enqueue(agent, batch, eps)
    p, ws = (lambda t: t.data_ptr()), updater._offpolicy_workspace(B)
    mean, std = updater.norm_tensors()
    gpu, d_eps = {k: v.cuda() for k, v in batch.items()}, eps.cuda()

    def raw(entry, *more):
        """The entry by itself (no optimizer step behind it) on sums pre-filled with a pattern: the padding of the weight rows, which no
        entry writes, keeps it."""
        updater.grad_sums.fill_(-12345.0)
        status = getattr(lib, entry)(
            p(updater._policy_params()), p(m.flat_target_critics.flat), p(updater.flat.flat), p(mean), p(std),
            updater.norm_clip(), p(gpu['observations']), p(gpu['actions']), p(gpu['next_observations']),
            p(gpu['rewards']), p(gpu['discounts']), p(d_eps), p(updater.values), p(updater.grad_sums), B, O,
            updater.hidden, A, NA, float(noise.scale), float(noise.clip), *more, p(ws), ws.numel(),
            torch.cuda.current_stream().cuda_stream)
        assert status == 0, lib.tonic_last_error().decode()
        torch.cuda.synchronize()
        sums = updater.grad_sums.clone().view(torch.int32)
        updater.grad_sums.zero_()
        return sums
    unweighted = raw('tonic_twin_distributional_q_grad')
    assert float((unweighted.view(torch.float32) != -12345.0).float().mean()) > 0.5
    assert torch.equal(raw('tonic_weighted_twin_distributional_q_grad', None, None), unweighted), \
        'NULL / NULL moved the bits'
    alone = _enqueue(agent, batch, eps, sample_losses=torch.zeros(B, device='cuda'))
    assert torch.equal(alone.view(torch.int32), plain.view(torch.int32))     # (the losses alone move nothing)

    out = td4_ref.critic_targets(nets, d, eps, noise.scale, noise.clip)
    assert td4_ref.precondition(out, nets.values, B)
    loss_1, loss_2, q1, q2 = td4_ref.critic_terms(nets, d, out['targets'])
    w64 = weights.double()
    (w64 * (loss_1 + loss_2)).mean().backward()
    losses = torch.full((B + 2,), float('nan'), device='cuda')
    sums = _enqueue(agent, batch, eps, weights=weights.cuda(), sample_losses=losses[1:B + 1])
    stats = sums[updater.count:].cpu().numpy()
    assert stats[5] == B and not stats[[3, 4, 6, 7]].any() and bool(torch.isnan(losses[[0, B + 1]]).all())
    leaves = nets.params['critic_1'] + nets.params['critic_2']
    err = _check(_grad_sums([m.critic_1, m.critic_2], sums, B), leaves, [f'critic tensor {i}' for i in range(len(leaves))])
    terms = (loss_1 + loss_2).detach()
    _check_stat(stats[0] / B, (w64 * terms).mean(), w64 * terms, 'weighted loss')
    _check_stat(stats[1] / B, q1.mean(), q1, 'q1')                         # (unweighted)
    _check_stat(stats[2] / B, q2.mean(), q2, 'q2')
    _check([losses[1:B + 1]], [terms.numpy()], ['sample losses'])
    print(f'td4 weighted {sizes} B={B} NA={NA}: largest relative error {err:.2e}')


# ---------------------------------------------------------------- whole update calls

ROWS, W, BATCH, ITERATIONS = 140, 3, 20, 6        # size 400 -> 133 rows of 3: the last 7 stores wrap


def _filled(kind, seed, replay):
    agent = _agent(O, A, (32, 32), 'ReLU', BATCH, 51, twin=kind == 'td4', replay=replay, seed=seed)
    rng = np.random.RandomState(seed)
    _set_normalizer(agent, rng.normal(size=O) * 0.3, np.exp(rng.uniform(-0.5, 0.5, O)))
    if kind == 'td4':
        _spread_targets(agent, balance=False)
    host = dict(observations=rng.normal(size=(ROWS, W, O)), actions=rng.uniform(-1, 1, (ROWS, W, A)),
                next_observations=rng.normal(size=(ROWS, W, O)), rewards=rng.normal(size=(ROWS, W)) * 2,
                resets=rng.uniform(size=(ROWS, W)) < 0.1, terminations=rng.uniform(size=(ROWS, W)) < 0.05)
    for t in range(ROWS):
        replay.store(**{k: torch.as_tensor(np.asarray(v[t], np.float32)).cuda() for k, v in host.items()})
    torch.cuda.synchronize()
    return agent


def _state(agent):
    """Everything an update moves, as bytes."""
    tensors = [agent.model.flat_online, agent.model.flat_target]
    for updater in (agent.critic_updater, agent.actor_updater):
        tensors += [updater.exp_avg, updater.exp_avg_sq, updater.state]
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in tensors]


def _host_loop(agent, uniforms, eps):
    """The update call step by step, nothing captured: per iteration the sample, the single-batch gather, the weighted
    critic step, the priority update and, when due, the actor step.  Returns (indices, weights, losses, infos)."""
    replay, critic, actor, model = agent.replay, agent.critic_updater, agent.actor_updater, agent.model
    device = dict(dtype=torch.float32, device='cuda')
    d_uniforms, d_eps = torch.as_tensor(uniforms).cuda(), torch.as_tensor(eps).cuda()
    indices = torch.zeros(uniforms.shape, dtype=torch.int64, device='cuda')
    weights, losses = torch.zeros(uniforms.shape, **device), torch.zeros(uniforms.shape, **device)
    infos = torch.zeros(2, len(uniforms), 8, **device)
    for it in range(len(uniforms)):
        replay.sample(d_uniforms[it], indices[it], weights[it])
        batch = replay.gather(indices[it])
        critic.enqueue(batch, d_eps[it, 0], infos[0, it], None, weights=weights[it], sample_losses=losses[it])
        replay.update_priorities(indices[it], losses[it])
        if agent._actor_due(it):
            actor.enqueue(batch['observations'], None, infos[1, it], None,
                          (model.flat_target, model.flat_online, 0, model.target_coeff))
    torch.cuda.synchronize()
    return indices.cpu().numpy(), weights.cpu().numpy(), losses.cpu().numpy(), infos.cpu().numpy()


@pytest.mark.parametrize('kind', ['d4pg', 'td4'])
def test_update_call(lib, kind, monkeypatch):
    from tonic_amd.replays import PrioritizedBuffer

    def replay():
        return PrioritizedBuffer(size=400, return_steps=5, batch_iterations=ITERATIONS, batch_size=BATCH)
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH', raising=False)
    captured = _filled(kind, 3, replay())
    monkeypatch.setenv('TONIC_AMD_NO_GRAPH', '1')
    eager = _filled(kind, 3, replay())
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH')
    assert _state(captured) == _state(eager) and captured.replay.capacity == 399
    assert torch.equal(captured.replay.tree, eager.replay.tree)
    max_leaf, levels = _read_tree(captured.replay)
    assert max_leaf == 1.0 and (levels == 1.0).all() and captured.replay.size == 133      # every row stored: full
    tree = prioritized_ref.Tree(399, levels, max_leaf)
    rng, graph = np.random.RandomState(5), None
    for call in range(2):
        uniforms = captured.replay.sample_uniforms()
        assert uniforms.shape == (ITERATIONS, BATCH) and uniforms.dtype == np.float64
        eps = rng.normal(size=(ITERATIONS, 1, BATCH, A)).astype(np.float32)
        infos = captured.enqueue_update(uniforms, eps).cpu().numpy()
        slot = captured._u.slot
        assert slot.graph is not None and (graph is None or slot.graph is graph), 'the second call captured again'
        graph = slot.graph
        indices, weights, losses, eager_infos = _host_loop(eager, uniforms, eps)
        assert np.array_equal(slot.indices.cpu().numpy(), indices)
        assert np.array_equal(slot.weights.cpu().numpy(), weights)
        assert np.array_equal(slot.sample_losses.cpu().numpy(), losses)
        assert np.array_equal(infos, eager_infos)
        assert _state(captured) == _state(eager), f'call {call}: the captured update and the host loop differ'
        assert torch.equal(captured.replay.tree, eager.replay.tree)
        due = [bool(captured._actor_due(it)) for it in range(ITERATIONS)]
        assert (infos[1][:, 6] > 0).tolist() == due and np.isfinite(infos).all()
        # the NumPy tree, fed with the read-back losses, draws the same indices at every iteration
        for it in range(ITERATIONS):
            drawn = [tree.descend(u) for u in uniforms[it]]
            assert min(margin for _, margin in drawn) >= 1e-7, 'a draw too close to a boundary to decide (the seed)'
            assert [index for index, _ in drawn] == indices[it].tolist(), (call, it)
            want = tree.weights(indices[it], captured.replay.beta)
            assert np.abs(weights[it] - want).max() <= 1e-5 * want.max()
            assert (losses[it] > 0).all()
            np.testing.assert_allclose(infos[0][it, 0], np.sum(weights[it].astype(np.float64) * losses[it]) / BATCH,
                                       rtol=1e-5)                           # critic/loss: the weighted mean
            tree.update(indices[it], losses[it], captured.replay.alpha, captured.replay.epsilon)
    max_leaf, levels = _read_tree(captured.replay)
    np.testing.assert_allclose(levels, tree.leaves, rtol=2e-6)
    assert max_leaf == tree.max_leaf or abs(max_leaf - tree.max_leaf) <= 2e-6 * max_leaf
    assert max_leaf >= levels.max()


def _read_tree(replay):
    raw = replay.tree.cpu().numpy()
    offset = prioritized_ref.level_offsets(replay.capacity)[0]
    leaves = np.frombuffer(raw[offset:offset + 4 * replay.capacity].tobytes(), np.float32).astype(np.float64)
    return np.frombuffer(raw[:4].tobytes(), np.float32)[0], leaves


def test_generator_api_and_stores(lib):
    """`get` with 'indices' and 'weights', `update_priorities` between two batches, a reserved row's priority."""
    from tonic_amd.replays import PrioritizedBuffer
    replay = PrioritizedBuffer(size=400, batch_iterations=3, batch_size=BATCH, alpha=1.0, epsilon=0.0)
    agent = _filled('d4pg', 4, replay)
    seen = []
    for batch in replay.get('observations', 'rewards', 'indices', 'weights', steps=7):
        assert set(batch) == {'observations', 'rewards', 'indices', 'weights'}
        indices = batch['indices'].cpu().numpy()
        stored = replay.buffers['rewards'].reshape(-1)[batch['indices']]
        assert torch.equal(batch['rewards'], stored) and batch['observations'].shape == (BATCH, O)
        assert (batch['weights'] <= 1).all() and (batch['weights'] > 0).all()
        seen.append(indices)
        # everything drawn so far gets no priority at all: it is never drawn again
        replay.update_priorities(batch['indices'], torch.zeros(BATCH, device='cuda'))
    assert replay.last_steps == 7 and len(seen) == 3
    flat = np.concatenate(seen)
    assert not np.intersect1d(seen[1], seen[0]).size and not np.intersect1d(seen[2], flat[:2 * BATCH]).size
    max_leaf, leaves = _read_tree(replay)
    assert (leaves[np.unique(flat)] == 0).all() and max_leaf == 1.0
    # a reserved row (its data write rides in a later launch) starts at max_leaf like a stored one
    row = replay.index
    replay.update_priorities(torch.arange(row * W, (row + 1) * W, device='cuda'), torch.zeros(W, device='cuda'))
    assert (_read_tree(replay)[1][row * W:(row + 1) * W] == 0).all()
    assert replay.reserve_row() == row and replay.index == row + 1
    torch.cuda.synchronize()
    assert (_read_tree(replay)[1][row * W:(row + 1) * W] == 1.0).all()
    agent.close()


# ---------------------------------------------------------------- refusals and non-regression

def test_sac_on_a_prioritized_buffer_is_refused_by_name(lib):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    from tonic_amd.replays import PrioritizedBuffer
    agent = tt.agents.SAC(replay=PrioritizedBuffer())
    with pytest.raises(NotImplementedError) as refusal:
        agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    text = str(refusal.value)
    assert 'TwinCriticSoftQLearning' in text and 'DistributionalDeterministicQLearning' in text
    assert 'TwinCriticDistributionalDeterministicQLearning' in text and 'PrioritizedBuffer' in text


def uniform_update_digest():
    """sha256 of everything two update calls of D4PG on a uniform Buffer move and log (seeded; W = 3, B = 20, 6
    iterations, 5-step returns).  Imports nothing this file's other tests need, so that the parent commit can run it."""
    import tonic_amd
    replay = tonic_amd.replays.Buffer(size=400, return_steps=5, batch_iterations=ITERATIONS, batch_size=BATCH)
    agent = _filled('d4pg', 3, replay)
    digest = hashlib.sha256()
    for _ in range(2):
        indices = replay.sample_indices()
        eps = np.zeros((ITERATIONS, 1, BATCH, A), np.float32)
        infos = agent.enqueue_update(indices, eps)
        digest.update(infos.cpu().numpy().tobytes())
        for part in _state(agent):
            digest.update(part)
    agent.close()
    return dict(sha256=digest.hexdigest())


def test_uniform_buffer_update_keeps_the_parents_bits(lib):
    """A D4PG update on the uniform Buffer gives the bits the parent commit gave: its route, its launches' results and
    its logs are untouched by the prioritized route."""
    with open(GOLDEN) as golden:
        recorded = json.load(golden)
    assert uniform_update_digest()['sha256'] == recorded['sha256']
