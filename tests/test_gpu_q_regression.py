"""GPU tests of QRegression: tonic_q_regression_grad and the updater against tests/q_regression_ref.py.

Gradient sums are held by the convention of tests/test_gpu_offpolicy_grads.py (`_check`): every tensor to 1e-5 of
its largest element, the statistic slot to the count B, the logged loss and q to float64 at rtol 1e-5 with the mean
absolute term as the scale.  L1, smooth-L1 and Huber have a kink in |q - y|: a float32 q that differs from the
float64 one in its last bits could fall on the other side of it.  So the returns of every case are the float64 q
minus an error from a fixed list (`ERRORS` times the rule's threshold), and `_precondition` asserts ON THE REFERENCE
ALONE that every row's |q - y| is at least 1e-3 away from the kink, with rows on both sides of it and of both signs;
no row is left out of a comparison.

Every test prints the largest relative error it saw."""
import copy
import ctypes

import numpy as np
import pytest

import q_regression_ref as ref
from test_gpu_offpolicy_grads import _Images, _check, _check_stat
from test_gpu_offpolicy_torsos import _grad_sums

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ERRORS = (0.3, -0.4, 1.6, -2.5, 0.7, -0.6, 3.0, -1.4)      # q - y in units of the rule's threshold (0.5 without one)


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def f32(a):
    return torch.as_tensor(np.asarray(a, np.float32))


# ---------------------------------------------------------------- models, batches and the raw entry

def _model(O, A, sizes, activation='ReLU', clip=None, ranged=None, seed=9, container=None, actor_sizes=None,
           device='cuda', normalizer=True):
    """A packed model on the device with a non-trivial MeanStd (`normalizer` False: none at all); `ranged` =
    (low, high) of a Return normaliser."""
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    act = getattr(torch.nn, activation)
    torch.manual_seed(seed)
    container = container or tt.models.ActorCriticWithTargets
    model = container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(actor_sizes or sizes, act),
                              head=tt.models.DeterministicPolicyHead()),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                                head=tt.models.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd(clip=clip) if normalizer else None,
        return_normalizer=tt.normalizers.Return(0.99) if ranged else None)
    model.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)))
    rng = np.random.RandomState(O * 7 + A)
    with torch.no_grad():
        if normalizer:
            model.observation_normalizer._mean.copy_(f32(rng.normal(size=O) * 0.3))
            model.observation_normalizer._std.copy_(f32(np.exp(rng.uniform(-0.5, 0.5, O))))
        if ranged:
            model.return_normalizer._low.fill_(ranged[0])
            model.return_normalizer._high.fill_(ranged[1])
    return model.pack(device)


def _updater(model, loss=('mse', None), **arguments):
    import tonic_amd.torch as tt
    updater = tt.updaters.QRegression(loss=ref.torch_loss(*loss), **arguments)
    updater.initialize(model)
    return updater


def _reference(model, activation, batch, loss=('mse', None), dtype=torch.float64):
    norm, ret = model.observation_normalizer, model.return_normalizer
    low, high = (ret._low, ret._high) if ret else (None, None)
    mean, std, clip = (norm._mean, norm._std, norm.clip) if norm else (None, None, None)
    return ref.step(model.critic.state_dict(), batch['observations'], batch['actions'], batch['returns'], activation,
                    loss, mean, std, clip, low, high, dtype=dtype)


def _batch(model, activation, B, O, A, loss=('mse', None), seed=0, spread=1.0):
    """Observations, actions and the returns: the float64 q minus ERRORS times the rule's threshold."""
    rng = np.random.RandomState(seed + 31 * B)
    batch = dict(observations=f32(rng.normal(size=(B, O)) * spread), actions=f32(rng.uniform(-1, 1, (B, A))),
                 returns=torch.zeros(B))
    q = _reference(model, activation, batch)['values']
    unit = ref.kink(*loss) or 0.5
    errors = torch.as_tensor([ERRORS[i % len(ERRORS)] for i in range(B)], dtype=torch.float64) * unit
    batch['returns'] = (q - errors).float()
    return batch


def _precondition(out, batch, loss, B):
    """On the float64 reference alone: every row at least 1e-3 from the kink; both sides and both signs present."""
    kink = ref.kink(*loss)
    if kink is None:
        return
    e = out['values'] - batch['returns'].double()
    assert float((e.abs() - kink).abs().min()) >= 1e-3, float((e.abs() - kink).abs().min())
    assert B >= 4 and (e > 0).any() and (e < 0).any()
    if kink > 0:
        for sign in (1, -1):
            assert ((sign * e > 0) & (e.abs() < kink)).any() and ((sign * e > 0) & (e.abs() > kink)).any()


def _entry(updater, batch):
    """One call of tonic_q_regression_grad as the updater makes it, without the optimizer step: the gradient sums
    and statistics (a clone)."""
    from tonic_amd import _lib
    gpu = {k: v.cuda().contiguous() for k, v in batch.items()}
    B = gpu['observations'].shape[0]
    ws = updater._offpolicy_workspace(B)
    mean, std = updater.norm_tensors()
    p = _lib.ptr
    updater.grad_sums.zero_()                             # (the padding floats are nobody's to write)
    _lib.check(updater.lib.tonic_q_regression_grad(
        p(updater.flat.flat), p(mean), p(std), updater.norm_clip(), p(gpu['observations']), p(gpu['actions']),
        p(gpu['returns']), p(updater.grad_sums), B, updater.observation_size, updater.hidden, updater.action_size,
        ctypes.addressof(updater.loss_rule), *updater.range_pointers(), p(ws), ws.numel(), _lib.current_stream()),
        'tonic_q_regression_grad')
    torch.cuda.synchronize()
    return updater.grad_sums.clone()


def _padding(critic, block):
    """The floats of a critic's flat block that belong to no tensor (row padding, slot padding)."""
    from tonic_amd.torch.models import FlatNetwork
    rest, at = block.clone(), 0
    for p, n, ld in FlatNetwork.slots([critic], padded=True):
        if ld:
            rest[at:at + n].view(p.shape[0], ld)[:, :p.shape[1]] = 0
        else:
            rest[at:at + p.numel()] = 0
        at += n
    assert at == block.numel()
    return rest


def _compare(model, updater, activation, batch, loss, label):
    """The entry's sums against the float64 restatement, the precondition asserted first."""
    B = batch['observations'].shape[0]
    out = _reference(model, activation, batch, loss)
    _precondition(out, batch, loss, B)
    sums = _entry(updater, batch)
    stats = sums[updater.count:].cpu().numpy()
    assert stats[5] == B and not stats[[2, 3, 4, 6, 7]].any(), stats
    got = _grad_sums([model.critic], sums, B)
    err = _check(got, out['params'], [f'critic tensor {i}' for i in range(len(got))])
    _check_stat(stats[0] / B, out['loss'], out['terms'], 'loss')
    _check_stat(stats[1] / B, out['values'].mean(), out['values'], 'q')
    assert not _padding(model.critic, sums[:updater.count]).any()      # (the layout's padding floats: zero gradient)
    print(f'q regression {label}: largest relative error {err:.2e}')
    return out, sums


# ---------------------------------------------------------------- 1. gradient sums against float64

BASE = dict(O=10, A=6, sizes=(32, 32), activation='ReLU', B=17, loss=('mse', None), clip=None, images=1)
AXES = [('B=%d' % B, dict(B=B)) for B in (1, 15, 16, 100)] + \
    [('O+A=%d+%d' % (O, A), dict(O=O, A=A)) for O, A in ((1, 1), (14, 1), (11, 6), (33, 9))] + \
    [('float32-one-launch', dict(images=0)), ('beyond-the-images', dict(sizes=(272, 272))),
     ('tanh40', dict(sizes=(40,), activation='Tanh')), ('relu24x40', dict(sizes=(24, 40))),
     ('elu64x48x32', dict(sizes=(64, 48, 32), activation='ELU')),
     ('tanh16x4', dict(sizes=(16, 16, 16, 16), activation='Tanh')),
     ('no-normaliser', dict(normalizer=False)), ('no-normaliser-layered', dict(normalizer=False, sizes=(24, 40))),
     ('clip-active', dict(clip=1.0, spread=2.0)),
     ('base', dict())] + \
    [('%s-%s' % loss, dict(loss=loss)) for loss in (('l1', None), ('smooth_l1', 0.5), ('smooth_l1', 2.0),
                                                   ('smooth_l1', 0.0), ('huber', 0.5), ('huber', 2.0))] + \
    [('huber-layered', dict(loss=('huber', 0.5), sizes=(24, 40))), ('l1-float32', dict(loss=('l1', None), images=0))]


@pytest.mark.parametrize('label,change', AXES, ids=[label for label, _ in AXES])
def test_grad_sums_vs_float64(lib, label, change):
    """Each axis against the base case (O + A = 16, B = 17: a ragged second tile, the (32, 32) ReLU torso on the
    weight images, MSE, a MeanStd with mean and std): batch sizes around the 16-row tile, input widths one below, at
    and above a multiple of 16, the three routes, four layer-by-layer torsos, the four losses, a model without an
    observation normaliser and one whose clip binds on a tenth of the elements at least."""
    case = dict(BASE, **change)
    O, A, B, sizes, activation, loss = (case[k] for k in ('O', 'A', 'B', 'sizes', 'activation', 'loss'))
    with _Images(lib, case['images']):
        model = _model(O, A, sizes, activation, clip=case['clip'], normalizer=case.get('normalizer', True))
        updater = _updater(model, loss)
        assert updater.stock is False and (updater.hidden == sizes[0]) == (len(sizes) == 2 and sizes[0] == sizes[1])
        batch = _batch(model, activation, B, O, A, loss, spread=case.get('spread', 1.0))
        if case['clip']:
            norm = model.observation_normalizer
            x = (batch['observations'] - norm._mean.cpu()) / norm._std.cpu()
            assert float((x.abs() > case['clip']).float().mean()) > 0.1
        _compare(model, updater, activation, batch, loss, label)


# ---------------------------------------------------------------- 2. the squashed head

RANGES = [(-3.0, 7.0), (2.0, 9.0)]


def _row_values(updater, batch):
    """Every row's value as the kernels publish it: the q statistic of single-row calls."""
    B = batch['observations'].shape[0]
    return np.array([float(_entry(updater, {k: v[r:r + 1] for k, v in batch.items()})[updater.count + 1])
                     for r in range(B)])


@pytest.mark.parametrize('route', ['images', 'float32', 'layered'])
@pytest.mark.parametrize('loss', [('mse', None), ('huber', 0.5)], ids=['mse', 'huber'])
def test_squashed_head_vs_float64(lib, route, loss):
    """The check of test 1 under a Return normaliser with (_low, _high) = (-3, 7), then — the same model, the range
    overwritten on the device — with (2, 9), which does not contain 0; every row's value lies strictly inside the
    range.  (Seen on the MI355X: at most 2.5e-6 under MSE and 6.3e-6 under Huber with (2, 9) on every route — there
    an error q - y of 0.15 is the difference of values near 5.3, each rounded to 2^-24 of itself.)"""
    O, A, B = 10, 6, 17
    sizes = (24, 40) if route == 'layered' else (32, 32)
    with _Images(lib, int(route == 'images')):
        model = _model(O, A, sizes, ranged=RANGES[0])
        updater = _updater(model, loss)
        assert updater.stock is False and None not in updater.range_pointers()
        for low, high in RANGES:
            with torch.no_grad():
                model.return_normalizer._low.fill_(low)
                model.return_normalizer._high.fill_(high)
            batch = _batch(model, 'ReLU', B, O, A, loss, seed=3)
            out, _ = _compare(model, updater, 'ReLU', batch, loss, f'{route} {loss[0]} range ({low}, {high})')
            if loss[0] == 'mse':
                values = _row_values(updater, batch)
                assert (values > low).all() and (values < high).all(), values
                np.testing.assert_allclose(values, out['values'].numpy(), rtol=0, atol=1e-5 * max(abs(low), abs(high)))


def test_captured_graph_follows_the_range(lib):
    """A graph captured under (-3, 7) and replayed after _low / _high were overwritten on the device gives the bits
    of a fresh eager call under the new range: the range is read by the kernels, nothing is captured again."""
    from tonic_amd import _lib
    O, A, B = 10, 6, 17
    model = _model(O, A, (32, 32), ranged=RANGES[0])
    updater = _updater(model, ('huber', 0.5))
    batch = _batch(model, 'ReLU', B, O, A, ('huber', 0.5), seed=3)
    gpu = {k: v.cuda() for k, v in batch.items()}
    first = _entry(updater, gpu)                          # (also: the workspace and the kernels' attributes exist)
    ws, (mean, std), p = updater._offpolicy_workspace(B), updater.norm_tensors(), _lib.ptr
    graph = torch.cuda.CUDAGraph()
    with _lib.capturing(graph):
        _lib.check(updater.lib.tonic_q_regression_grad(
            p(updater.flat.flat), p(mean), p(std), updater.norm_clip(), p(gpu['observations']), p(gpu['actions']),
            p(gpu['returns']), p(updater.grad_sums), B, O, updater.hidden, A, ctypes.addressof(updater.loss_rule),
            *updater.range_pointers(), p(ws), ws.numel(), _lib.current_stream()), 'tonic_q_regression_grad')
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(updater.grad_sums, first)
    with torch.no_grad():
        model.return_normalizer._low.fill_(RANGES[1][0])
        model.return_normalizer._high.fill_(RANGES[1][1])
    updater.grad_sums.zero_()
    graph.replay()
    torch.cuda.synchronize()
    replayed = updater.grad_sums.clone()
    fresh = _entry(updater, gpu)
    assert torch.equal(replayed, fresh) and not torch.equal(replayed, first)


# ---------------------------------------------------------------- 3. agreement with the DDPG critic step

def _ddpg_sums(lib, model, updater, batch, H):
    """tonic_twin_q_grad_ranged, kind 2, with rewards = returns and discounts = 0: y = r + 0 tq = r."""
    from tonic_amd import _lib
    gpu = {k: v.cuda().contiguous() for k, v in batch.items()}
    B, O, A = gpu['observations'].shape[0], updater.observation_size, updater.action_size
    need = lib.tonic_offpolicy_workspace_bytes(B, O, A, H)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    sums = torch.zeros_like(updater.grad_sums)
    mean, std = updater.norm_tensors()
    next_observations = torch.randn(B, O, device='cuda')
    zeros, p = torch.zeros(B, device='cuda'), _lib.ptr
    _lib.check(lib.tonic_twin_q_grad_ranged(
        2, p(model.flat_target_actor.flat), p(model.flat_target_critics.flat), p(model.flat_critics.flat), p(mean),
        p(std), updater.norm_clip(), p(gpu['observations']), p(gpu['actions']), p(next_observations),
        p(gpu['returns']), p(zeros), None, p(sums), B, O, H, A, 0.0, 0.0, 0.0, ctypes.addressof(updater.loss_rule),
        *updater.range_pointers(), p(ws), need, _lib.current_stream()), 'tonic_twin_q_grad_ranged')
    torch.cuda.synchronize()
    return sums


@pytest.mark.parametrize('ranged', [False, True], ids=['plain', 'ranged'])
@pytest.mark.parametrize('route', ['images', 'float32', 'layered'])
def test_bit_identical_with_the_ddpg_critic_step(lib, route, ranged):
    """On each route, with and without the range, the gradient sums and the statistics are the bits of the DDPG
    critic step with zero discounts (finite target networks): every network's tiles are independent of how many
    networks a launch carries."""
    O, A, B = 11, 6, 37
    sizes = (24, 40) if route == 'layered' else (32, 32)
    loss = ('huber', 0.5) if ranged else ('mse', None)
    with _Images(lib, int(route == 'images')):
        model = _model(O, A, sizes, ranged=RANGES[0] if ranged else None)
        updater = _updater(model, loss)
        batch = _batch(model, 'ReLU', B, O, A, loss, seed=5)
        got = _entry(updater, batch)
        want = _ddpg_sums(lib, model, updater, batch, updater.hidden)
    assert torch.isfinite(want).all() and float(want[:updater.count].abs().max()) > 0
    different = int((got != want).sum())
    print(f'q regression vs DDPG critic step, {route} {"ranged" if ranged else "plain"}: {different} of '
          f'{got.numel()} floats differ')
    assert torch.equal(got, want)


@pytest.mark.parametrize('route', ['images', 'float32', 'layered'])
def test_nothing_is_written_past_the_query_or_the_sums(lib, route):
    """A workspace of exactly the query's size with 4 KiB of a pattern behind it, and a gradient block with 64
    patterned floats behind its 8 statistics: the entry leaves both patterns alone and gives the bits it gives in the
    updater's own buffers."""
    from tonic_amd import _lib
    O, A, B = 11, 6, 37
    sizes = (24, 40) if route == 'layered' else (32, 32)
    with _Images(lib, int(route == 'images')):
        model = _model(O, A, sizes, ranged=RANGES[0])
        updater = _updater(model, ('huber', 0.5))
        batch = _batch(model, 'ReLU', B, O, A, ('huber', 0.5), seed=5)
        want = _entry(updater, batch)
        need, count, p = lib.tonic_q_regression_workspace_bytes(B, O, A, updater.hidden), updater.count, _lib.ptr
        ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
        sums = torch.zeros(count + 8 + 64, device='cuda')
        sums[count + 8:] = 12345.0
        gpu = {k: v.cuda() for k, v in batch.items()}
        mean, std = updater.norm_tensors()
        _lib.check(lib.tonic_q_regression_grad(
            p(updater.flat.flat), p(mean), p(std), updater.norm_clip(), p(gpu['observations']), p(gpu['actions']),
            p(gpu['returns']), p(sums), B, O, updater.hidden, A, ctypes.addressof(updater.loss_rule),
            *updater.range_pointers(), p(ws), need, _lib.current_stream()), 'tonic_q_regression_grad')
        torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()) and bool((sums[count + 8:] == 12345.0).all())
    assert torch.equal(sums[:count + 8], want)


# ---------------------------------------------------------------- 4. additivity for shards

def test_sums_add_up_over_parts_of_a_batch(lib):
    O, A, B = 10, 6, 48
    model = _model(O, A, (32, 32))
    updater = _updater(model)
    batch = _batch(model, 'ReLU', B, O, A)
    whole = _entry(updater, batch)
    parts = [_entry(updater, {k: v[a:b].contiguous() for k, v in batch.items()}) for a, b in ((0, 20), (20, 48))]
    count = updater.count
    assert [float(part[count + 5]) for part in parts] == [20.0, 28.0] and float(whole[count + 5]) == 48.0
    total = parts[0] + parts[1]
    err = _check(_grad_sums([model.critic], total, 1), _grad_sums([model.critic], whole.double().cpu(), 1),
                 [f'critic tensor {i}' for i in range(6)])
    out = _reference(model, 'ReLU', batch)
    _check_stat(float(total[count]) / B, out['loss'], out['terms'], 'loss')
    _check_stat(float(total[count + 1]) / B, out['values'].mean(), out['values'], 'q')
    print(f'q regression parts of a batch: largest relative error {err:.2e}')


def test_shard_protocol(lib):
    """A rank that drew 20 of a global batch of 48 and one that drew none: enqueue(part, n_global = 48) is the
    entry's sums stepped with grad_scale 1 / 48, enqueue_empty(row, 48) is a step on zero sums — the same launches,
    parameters, optimizer state and info row as DeterministicQLearning.enqueue_empty makes on the same model."""
    import tonic_amd.torch as tt
    O, A = 10, 6
    results = []
    for how in ('enqueue', 'by hand', 'empty', 'ddpg empty'):
        model = _model(O, A, (32, 32))
        updater = _updater(model) if how != 'ddpg empty' else tt.updaters.DeterministicQLearning()
        if how == 'ddpg empty':
            updater.initialize(model)
        batch = {k: v[:20].contiguous() for k, v in _batch(model, 'ReLU', 48, O, A).items()}
        info = torch.full((8,), -1.0, device='cuda')
        if how == 'enqueue':
            updater.enqueue({k: v.cuda() for k, v in batch.items()}, info, n_global=48)
        elif how == 'by hand':
            sums = _entry(updater, batch)
            updater.optim.enqueue(updater.flat.flat, sums, 1.0 / 48, info, 3)
        else:
            updater.enqueue_empty(info, 48)
        torch.cuda.synchronize()
        results.append((model.flat_online.cpu().numpy(), updater.slots.cpu().numpy(), updater.state.cpu().numpy(),
                        info.cpu().numpy()))
    for a, b in ((0, 1), (2, 3)):
        for got, want in zip(results[a], results[b]):
            assert np.array_equal(got, want, equal_nan=True)
    assert results[0][2][0] == 1 and results[2][2][0] == 1 and results[0][3][6] == 1.0
    assert not np.array_equal(results[0][0], results[2][0])           # (the part moved the critic, the empty step not)


# ---------------------------------------------------------------- 5. the whole updater

def _cpu_copy(model):
    critic = copy.deepcopy(model.critic).cpu()
    variables = [p for name, p in critic.named_parameters() if 'normalizer' not in name]
    for p in variables:
        p.data = p.data.clone().contiguous()
        p.requires_grad_(True)
    return critic, variables


UPDATER_CASES = [
    pytest.param(dict(), dict(), id='adam-default'),
    pytest.param(dict(sizes=(24, 40), ranged=RANGES[0]),
                 dict(loss=('huber', 0.5), optimizer=lambda p: torch.optim.SGD(p, lr=1e-2, momentum=0.9)),
                 id='sgd-momentum-huber-ranged-layered'),
    pytest.param(dict(), dict(gradient_clip=0.05), id='gradient-clip'),
    pytest.param(dict(sizes=(16,) * 5, activation='Tanh'), dict(loss=('smooth_l1', 0.5), stock=True), id='stock-five-layers'),
    pytest.param(dict(plain_container=True), dict(gradient_clip=0.05, stock=True), id='stock-actor-critic'),
]


@pytest.mark.parametrize('model_arguments,arguments', UPDATER_CASES)
def test_four_calls_match_float32_autograd(lib, model_arguments, arguments):
    """Four calls of QRegression.__call__ against float32 torch autograd on a CPU copy of the critic stepped by
    torch.optim: parameter deltas within atol 1e-5, the logged loss and q of every call within rtol 1e-5 / atol 1e-5
    (the bounds of tests/test_gpu_td4.py::test_update_call_matches_the_float32_restatement)."""
    import tonic_amd.torch as tt
    O, A, B = 10, 6, 37
    arguments, model_arguments = dict(arguments), dict(model_arguments)
    stock, loss = arguments.pop('stock', False), arguments.pop('loss', ('mse', None))
    activation = model_arguments.get('activation', 'ReLU')
    container = tt.models.ActorCritic if model_arguments.pop('plain_container', False) else None
    model = _model(O, A, model_arguments.pop('sizes', (32, 32)), container=container, **model_arguments)
    critic, variables = _cpu_copy(model)
    factory = arguments.get('optimizer') or (lambda p: torch.optim.Adam(p, lr=1e-3))
    optimizer, clip = factory(variables), arguments.get('gradient_clip', 0)
    updater = _updater(model, loss, **arguments)
    assert updater.stock is stock
    start = [p.detach().cpu().numpy().copy() for p in tt.models.trainable_variables(model.critic)]
    before = [p.detach().numpy().copy() for p in variables]
    worst, clipped = 0.0, 0
    for call in range(4):
        batch = _batch(model, activation, B, O, A, loss, seed=call)
        optimizer.zero_grad()
        values = critic(batch['observations'], batch['actions'])
        want = ref.loss_terms(values, batch['returns'], *loss).mean()
        want.backward()
        if clip > 0:
            clipped += float(torch.nn.utils.clip_grad_norm_(variables, clip)) > clip
        optimizer.step()
        infos = updater(*(batch[k].cuda() for k in ('observations', 'actions', 'returns')))
        np.testing.assert_allclose(float(infos['loss']), float(want.detach()), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(float(infos['q']), float(values.detach().mean()), rtol=1e-5, atol=1e-5)
    assert clipped == (4 if clip > 0 else 0)
    moved = 0.0
    for i, (p, q) in enumerate(zip(tt.models.trainable_variables(model.critic), variables)):
        got, want = p.detach().cpu().numpy() - start[i], q.detach().numpy() - before[i]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5, err_msg=f'tensor {i}')
        worst, moved = max(worst, float(np.abs(got - want).max())), max(moved, float(np.abs(want).max()))
    assert moved > 1e-3
    print(f'q regression four calls: largest |delta - reference| {worst:.2e} of deltas up to {moved:.2e}')


def test_graph_replay_of_enqueue_is_bit_identical_with_eager_launches(lib):
    """Three steps after a first eager one: launch by launch on one model, as three replays of ONE captured
    `enqueue` on another — parameters, optimizer state and info rows are the same bits."""
    from tonic_amd import _lib
    O, A, B = 10, 6, 37
    results = []
    for graphed in (False, True):
        model = _model(O, A, (32, 32), ranged=RANGES[0])
        updater = _updater(model, ('huber', 0.5), gradient_clip=0.05)
        batches = [_batch(model, 'ReLU', B, O, A, ('huber', 0.5), seed=s) for s in range(4)]
        static = {k: v.cuda() for k, v in batches[0].items()}
        info, rows = torch.zeros(8, device='cuda'), []
        updater.enqueue(static, info)
        torch.cuda.synchronize()
        graph = None
        if graphed:
            graph = torch.cuda.CUDAGraph()
            with _lib.capturing(graph):
                updater.enqueue(static, info)
        for batch in batches[1:]:
            for k, v in batch.items():
                static[k].copy_(v)
            if graphed:
                graph.replay()
            else:
                updater.enqueue(static, info)
            torch.cuda.synchronize()
            rows.append(info.cpu().numpy().copy())
        results.append((model.flat_online.cpu().numpy(), updater.slots.cpu().numpy(), updater.state.cpu().numpy(),
                        np.array(rows)))
    assert results[0][2][0] == 4 and np.isfinite(results[0][3]).all()
    for got, want in zip(results[1], results[0]):
        assert np.array_equal(got, want)


# ---------------------------------------------------------------- 6. non-finite data

@pytest.mark.parametrize('route', ['float32', 'layered'])
def test_nan_and_inf_returns_under_mse(lib, route):
    """One NaN and one inf return under MSE, against float32 torch autograd: the loss is NaN as torch's is, q is
    finite; a gradient element is finite exactly where torch's is — the hidden units on which neither row is active
    — and there it is the other rows' contribution (their dq is untouched), within 1e-5 of the tensor's largest
    finite element."""
    O, A, B = 10, 6, 17
    sizes = (24, 40) if route == 'layered' else (32, 32)
    with _Images(lib, 0):
        model = _model(O, A, sizes)
        updater = _updater(model)
        batch = _batch(model, 'ReLU', B, O, A)
        batch['returns'][3], batch['returns'][12] = float('nan'), float('inf')
        sums = _entry(updater, batch)
    out = _reference(model, 'ReLU', batch, dtype=torch.float32)
    stats = sums[updater.count:].cpu().numpy()
    assert np.isnan(stats[0]) and torch.isnan(out['loss']) and stats[5] == B
    np.testing.assert_allclose(stats[1] / B, float(out['values'].mean()), rtol=1e-5)
    finite_elements = 0
    for i, (g, want) in enumerate(zip(_grad_sums([model.critic], sums, B), out['grads'])):
        g, want = g.cpu().numpy(), want.numpy()
        assert np.array_equal(np.isfinite(g), np.isfinite(want)), f'tensor {i}'
        mask = np.isfinite(want)
        if mask.any():
            scale = max(np.abs(want[mask]).max(), 1e-30)
            np.testing.assert_allclose(g[mask], want[mask], rtol=0, atol=1e-5 * scale, err_msg=f'tensor {i}')
            finite_elements += int((mask & (want != 0)).sum())
    assert finite_elements > 0                            # (some unit is inactive on both rows: the test sees rows apart)


def test_nan_return_under_l1_contributes_no_gradient(lib):
    """Under L1 the gradient of a row is the sign of its error alone: 0 for a NaN error, -1 for y = +inf.  Every
    gradient is finite, as float32 torch's are, and the loss is NaN.  The weight and hidden-bias gradients are held
    to the float64 restatement; the head's bias gradient is the sum of the rows' signs — integers, which the kernels
    must give exactly (in torch it is a sum of +-1 / B that cancels to a rounding residue, no scale to compare to)."""
    O, A, B = 10, 6, 17
    model = _model(O, A, (32, 32))
    updater = _updater(model, ('l1', None))
    batch = _batch(model, 'ReLU', B, O, A, ('l1', None))
    batch['returns'][3], batch['returns'][12] = float('nan'), float('inf')
    sums = _entry(updater, batch)
    single = _reference(model, 'ReLU', batch, ('l1', None), dtype=torch.float32)
    assert np.isnan(float(sums[updater.count])) and torch.isnan(single['loss'])
    assert all(torch.isfinite(g).all() for g in single['grads'])
    out = _reference(model, 'ReLU', batch, ('l1', None))
    signs = torch.sign(out['values'] - batch['returns'].double())
    signs[torch.isnan(signs)] = 0.0
    assert signs[3] == 0 and signs[12] == -1 and signs.abs().sum() == B - 1
    err = _check(_grad_sums([model.critic], sums, B)[:5], out['params'][:5], [f'critic tensor {i}' for i in range(5)])
    assert float(_grad_sums([model.critic], sums, 1)[5]) == float(signs.sum())
    print(f'q regression L1 with a NaN row: largest relative error {err:.2e}')
