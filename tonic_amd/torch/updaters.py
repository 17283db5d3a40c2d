"""Learner updaters on the HIP engine — API of ``tonic/torch/updaters/{actors,critics}.py``.

``ClippedRatio`` (actors.py:53-112) and ``VRegression`` (critics.py:6-28) keep their
constructor arguments, ``initialize(model)`` and ``__call__`` returning a dict whose values
expose ``.numpy()``.  Internally one update is three asynchronous launches on the current
stream, with no host synchronisation:

    tonic_ppo_actor_grad / tonic_value_regression_grad   fused forward + loss + backward
    [all-reduce of the flat gradient-sum buffer over RCCL when world_size > 1]
    tonic_optimizer_step                                  flat optimizer step + logged statistics

The PPO agent drives them through ``enqueue`` for all 80 iterations and reads the
statistics back once; ``__call__`` (enqueue + read back) exists for drop-in compatibility.
"""
import ctypes
import math
import os
import types

import numpy as np
import torch

from tonic_amd import _lib

INFO_WIDTH = 8
ACTOR_INFO = ('loss', 'kl', 'entropy', 'clip_fraction', 'std', 'stop')


def adam_hyperparameters(factory, default_lr):
    """Reads lr / betas / eps from the reference-style ``optimizer=lambda params: Adam(...)``
    factory (actors.py:58-59) so user configs keep working; only plain Adam is fused."""
    if factory is None:
        return dict(lr=default_lr, betas=(0.9, 0.999), eps=1e-8)
    probe = factory([torch.nn.Parameter(torch.zeros(1))])
    if not isinstance(probe, torch.optim.Adam) or isinstance(probe, torch.optim.AdamW):
        raise NotImplementedError(f'only torch.optim.Adam is fused on the HIP engine, got {type(probe)}')
    d = probe.defaults
    if d.get('weight_decay', 0) != 0 or d.get('amsgrad', False) or d.get('maximize', False):
        raise NotImplementedError('Adam with weight_decay / amsgrad / maximize is not fused')
    return dict(lr=float(d['lr']), betas=tuple(float(b) for b in d['betas']), eps=float(d['eps']))


_FAMILY = {torch.optim.Adam: 'adam', torch.optim.AdamW: 'adamw', torch.optim.SGD: 'sgd',
           torch.optim.RMSprop: 'rmsprop'}


def optimizer_hyperparameters(factory, default_lr):
    """The rule behind the reference-style ``optimizer=lambda params: torch.optim.X(params, ...)`` factory
    (actors.py:58-59), probed like `adam_hyperparameters`: Adam (with weight_decay / amsgrad / maximize), AdamW, SGD
    (momentum, dampening, nesterov) and RMSprop (centered, momentum) run on the HIP engine (tonic_optimizer_step).
    -> dict(kind=, lr=, weight_decay=, maximize=, ...) with the rule's own keys,
    every number a Python float (float64) as torch keeps it.  Anything else is rejected by name."""
    if factory is None:
        return dict(kind='adam', lr=float(default_lr), betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                    amsgrad=False, maximize=False)
    probe = factory([torch.nn.Parameter(torch.zeros(1))])
    kind = _FAMILY.get(type(probe))
    if kind is None:
        raise NotImplementedError(
            f'{type(probe).__module__}.{type(probe).__name__} does not run on the HIP engine: the optimizers served '
            'are torch.optim.Adam, AdamW, SGD and RMSprop')
    if len(probe.param_groups) != 1:
        raise NotImplementedError(f'{type(probe).__name__} with {len(probe.param_groups)} parameter groups: one flat '
                                  'block has one set of hyper-parameters')
    d = probe.param_groups[0]
    if isinstance(d['lr'], torch.Tensor):
        raise NotImplementedError(f'{type(probe).__name__} with a tensor lr: the step takes a Python float')
    rule = dict(kind=kind, lr=float(d['lr']), weight_decay=float(d['weight_decay']), maximize=bool(d['maximize']))
    if kind in ('adam', 'adamw'):
        rule.update(betas=tuple(float(b) for b in d['betas']), eps=float(d['eps']), amsgrad=bool(d['amsgrad']))
    elif kind == 'sgd':
        rule.update(momentum=float(d['momentum']), dampening=float(d['dampening']), nesterov=bool(d['nesterov']))
    else:
        rule.update(alpha=float(d['alpha']), eps=float(d['eps']), momentum=float(d['momentum']),
                    centered=bool(d['centered']))
    return rule


def plain_adam(rule):
    """The rule `adam_hyperparameters` accepts: what tonic_adam_step_pair and the fused off-policy iteration
    compute (AdamW without decay is the same arithmetic).  Every rule, this one included, steps through
    tonic_optimizer_step otherwise."""
    return rule['kind'] in ('adam', 'adamw') and rule.get('weight_decay', 0.0) == 0 and \
        not rule.get('amsgrad', False) and not rule.get('maximize', False)


def optimizer_rule(rule):
    """`optimizer_hyperparameters`' dict as the tonic_optimizer_t of the C ABI."""
    betas = rule.get('betas', (0.0, 0.0))
    flags = sum(bit for name, bit in _lib.OPTIMIZER_FLAGS.items() if rule.get(name, False))
    return _lib.Optimizer(kind=_lib.OPTIMIZER_KINDS[rule['kind']], flags=flags, lr=rule['lr'], beta1=betas[0],
                          beta2=betas[1], eps=rule.get('eps', 0.0), weight_decay=rule['weight_decay'],
                          momentum=rule.get('momentum', 0.0), dampening=rule.get('dampening', 0.0),
                          alpha=rule.get('alpha', 0.0))


def _lr_segments():
    """class -> (kind, what `period`, `a`, `b` of tonic_lr_segment_t read from the scheduler object)."""
    s = torch.optim.lr_scheduler
    return {s.ConstantLR: ('constant', 'total_iters', 'factor', None),
            s.LinearLR: ('linear', 'total_iters', 'start_factor', 'end_factor'),
            s.ExponentialLR: ('exponential', None, 'gamma', None),
            s.StepLR: ('step', 'step_size', 'gamma', None),
            s.PolynomialLR: ('polynomial', 'total_iters', 'power', None),
            s.CosineAnnealingLR: ('cosine', 'T_max', 'eta_min', None)}


_LR_SERVED = 'the schedulers served are torch.optim.lr_scheduler.ConstantLR, LinearLR, ExponentialLR, StepLR, ' \
             'PolynomialLR, CosineAnnealingLR and a SequentialLR of two of them'


def _lr_segment(scheduler):
    name = f'{type(scheduler).__module__}.{type(scheduler).__qualname__}'
    entry = _lr_segments().get(type(scheduler))         # (exact classes: a subclass may compute anything)
    if entry is None:
        raise NotImplementedError(f'lr_scheduler={name} does not run on the HIP engine: {_LR_SERVED}')
    kind, period, a, b = entry
    values = {}
    for field, key in (('period', period), ('a', a), ('b', b)):
        value = getattr(scheduler, key) if key else 0
        if isinstance(value, torch.Tensor) or isinstance(value, bool) or not isinstance(value, (int, float)) or \
                (field == 'period' and value != int(value)) or not math.isfinite(value):
            raise NotImplementedError(f'{type(scheduler).__name__}({key}={value!r}) does not run on the HIP engine: '
                                      f'{"a whole number" if field == "period" else "a finite Python float"} is needed')
        values[field] = int(value) if field == 'period' else float(value)
    return _lib.LrSegment(kind=_lib.LR_KINDS[kind], **values)


def lr_schedule_rule(factory, optimizer_factory, default_lr):
    """The schedule behind the reference-style ``lr_scheduler=lambda optimizer: torch.optim.lr_scheduler.X(optimizer,
    ...)``, probed like `optimizer_hyperparameters` probes the optimizer: the factory is called on the probe
    optimizer, then the object's class and attributes are read.  -> the tonic_lr_schedule_t of the C ABI (None without
    a factory).  Exactly ConstantLR, LinearLR, ExponentialLR, StepLR, PolynomialLR, CosineAnnealingLR and a
    SequentialLR of two of them (the warm-up form) are served: the rate of step t is their closed form at t = the
    number of optimizer steps taken (include/tonic_hip.h).  Anything else is rejected by name.  Needs no device."""
    if factory is None:
        return None
    parameter = [torch.nn.Parameter(torch.zeros(1))]
    probe = optimizer_factory(parameter) if optimizer_factory is not None else \
        torch.optim.Adam(parameter, lr=default_lr)
    try:
        scheduler = factory(probe)
    except (ValueError, TypeError, KeyError, ZeroDivisionError) as error:      # (torch's own constructors' refusals)
        raise NotImplementedError(f'lr_scheduler: {type(error).__name__}: {error}') from error
    sequential = torch.optim.lr_scheduler.SequentialLR
    schedule = _lib.LrSchedule(count=1)
    if type(scheduler) is sequential:
        parts, milestones = list(scheduler._schedulers), list(scheduler._milestones)
        if len(parts) != 2:
            raise NotImplementedError(f'SequentialLR of {len(parts)} schedulers does not run on the HIP engine: '
                                      f'{_LR_SERVED}')
        if any(isinstance(part, sequential) for part in parts):
            raise NotImplementedError(f'a nested SequentialLR does not run on the HIP engine: {_LR_SERVED}')
        if isinstance(milestones[0], bool) or not isinstance(milestones[0], int):
            raise NotImplementedError(f'SequentialLR(milestones={milestones!r}): a whole number of steps is needed')
        schedule.count, schedule.milestone = 2, milestones[0]
        schedule.segment[0], schedule.segment[1] = _lr_segment(parts[0]), _lr_segment(parts[1])
    else:
        schedule.segment[0] = _lr_segment(scheduler)
    lib = _lib.load()
    if lib.tonic_lr_schedule_check(ctypes.byref(schedule)) != 0:
        raise NotImplementedError(f'lr_scheduler={type(scheduler).__name__}: {lib.tonic_last_error().decode()}')
    return schedule


def lr_schedule_value(schedule, lr, step):
    """The rate of the step taken after `step` steps from the base rate (tonic_lr_schedule_value: THE statement)."""
    return _lib.load().tonic_lr_schedule_value(ctypes.byref(schedule) if schedule is not None else None,
                                               float(lr), int(step))


_CRITIC_LOSSES = {torch.nn.MSELoss: ('mse', None), torch.nn.L1Loss: ('l1', None),
                  torch.nn.SmoothL1Loss: ('smooth_l1', 'beta'), torch.nn.HuberLoss: ('huber', 'delta')}


def critic_loss_rule(loss):
    """The reference-style ``loss=`` of the off-policy critic updaters (critics.py:58,142,189,243) as the
    tonic_critic_loss_t of the C ABI: exactly torch.nn.MSELoss (and None, the default), L1Loss, SmoothL1Loss(beta)
    and HuberLoss(delta) with reduction 'mean' run on the HIP engine; `param` is beta / delta as the float32 the
    kernels compare with.  A subclass, any other module or callable, or another reduction is rejected by name."""
    if loss is None:
        return _lib.CriticLoss()
    served = 'the critic losses served are torch.nn.MSELoss, L1Loss, SmoothL1Loss and HuberLoss with ' \
             "reduction='mean'"
    entry = _CRITIC_LOSSES.get(type(loss))
    if entry is None:
        name = f'{type(loss).__module__}.{type(loss).__qualname__}' if isinstance(loss, torch.nn.Module) else \
            repr(loss)
        raise NotImplementedError(f'loss={name} does not run on the HIP engine: {served}')
    if loss.reduction != 'mean':
        raise NotImplementedError(f"{type(loss).__name__}(reduction={loss.reduction!r}) does not run on the HIP "
                                  f'engine: {served}')
    kind, key = entry
    param = float(np.float32(getattr(loss, key))) if key else 0.0
    rule = _lib.CriticLoss(kind=_lib.CRITIC_LOSS_KINDS[kind], param=param)
    lib = _lib.load()
    if lib.tonic_critic_loss_check(ctypes.byref(rule)) != 0:
        raise NotImplementedError(f'loss={loss!r}: {lib.tonic_last_error().decode()}')
    return rule


def critic_loss_sum(rule, values, returns):
    """The SUM over the batch of the rule's loss terms as stock torch operators (the stock-torch updaters divide
    by the global batch size themselves)."""
    functional = torch.nn.functional
    if rule.kind == _lib.CRITIC_LOSS_KINDS['mse']:
        return ((values - returns) ** 2).sum()
    if rule.kind == _lib.CRITIC_LOSS_KINDS['l1']:
        return functional.l1_loss(values, returns, reduction='sum')
    if rule.kind == _lib.CRITIC_LOSS_KINDS['smooth_l1']:
        return functional.smooth_l1_loss(values, returns, reduction='sum', beta=rule.param)
    return functional.huber_loss(values, returns, reduction='sum', delta=rule.param)


def optimizer_slots(lib, rule, count, device):
    """(tonic_optimizer_t, its zeroed state buffers as ONE tensor of slots x count floats, None without state)."""
    packed = optimizer_rule(rule)
    slots = lib.tonic_optimizer_state_slots(ctypes.byref(packed))
    if slots < 0:
        raise NotImplementedError(f'{rule}: {lib.tonic_last_error().decode() or "not a rule of the family"}')
    return packed, (torch.zeros(slots * count, dtype=torch.float32, device=device) if slots else None)


class _OptimizerState:
    """One flat block's optimizer on the device: `rule`, the packed tonic_optimizer_t; `slots`, its state buffers as
    ONE tensor of slots x count floats (None for a rule without state); `state`, the int32 words {step, stop, -,
    arrivals}.  For Adam and AdamW `exp_avg` / `exp_avg_sq` are views of the first two slots (what
    tonic_adam_step_pair and the fused off-policy iteration take); None for SGD and RMSprop."""

    def __init__(self, lib, hyper, count, device, schedule=None):
        self.lib, self.count = lib, count
        self.schedule = schedule            # the packed tonic_lr_schedule_t of `lr_schedule_rule`, or None
        self.rule, self.slots = optimizer_slots(lib, hyper, count, device)
        self.state = torch.zeros(4, dtype=torch.int32, device=device)
        self.exp_avg = self.exp_avg_sq = None
        if hyper['kind'] in ('adam', 'adamw'):
            self.exp_avg, self.exp_avg_sq = self.slots[:count], self.slots[count:2 * count]

    def enqueue(self, params, grad_sums, grad_scale, info_row, stats_kind=0, kl_threshold=0.0, entropy_coeff=0.0,
                adv_stats=None, skip=None, targets=None, what='tonic_optimizer_step'):
        """The step of `params` (the block's `count` floats) from `grad_sums`.  `targets` = (flat target buffer,
        flat online buffer, offset of this block in them, coeff): the polyak update of ALL targets rides in the
        same launch."""
        polyak = (None, None, 0, 0, 0.0)
        if targets is not None:
            target, online, offset, coeff = targets
            assert online.data_ptr() + 4 * offset == params.data_ptr()
            polyak = (_lib.ptr(target), _lib.ptr(online), online.numel(), offset, float(coeff))
        step, scheduled = self.lib.tonic_optimizer_step, ()
        if self.schedule is not None:       # the rate of the step is formed on the device, at its own step count
            step, scheduled = self.lib.tonic_scheduled_optimizer_step, (ctypes.byref(self.schedule),)
            what = what.replace('tonic_optimizer_step', 'tonic_scheduled_optimizer_step')
        _lib.check(step(
            _lib.ptr(params), _lib.ptr(grad_sums), _lib.ptr(self.slots), _lib.ptr(self.state), self.count,
            grad_scale, ctypes.byref(self.rule), stats_kind, float(kl_threshold), float(entropy_coeff),
            _lib.ptr(adv_stats), _lib.ptr(info_row), skip, *polyak, *scheduled, _lib.current_stream()), what)

    def learning_rate(self, step=None):
        """The rate of the step taken after `step` steps (None: the device's count, one read-back: the next step's)."""
        return lr_schedule_value(self.schedule, self.rule.lr, int(self.state[0]) if step is None else step)


def fused_ppo_torso(torso):
    """The fused PPO kernels (csrc/mlp64x16.hip; layer by layer for wide observations / actions) serve the
    reference's default torso, MLP((64, 64), Tanh)."""
    return tuple(torso.sizes) == (64, 64) and torso.activation is torch.nn.Tanh


_TORSO_ACTIVATIONS = {torch.nn.Tanh: 1, torch.nn.ReLU: 2}


def hip_ppo_torso(torso):
    """(layers, sizes as a ctypes int32 array, activation code) when the layer-by-layer HIP path
    (csrc/mlpwide.hip, the tonic_*_torso entries) serves this ``MLP(sizes, activation)``: 1 .. 4 hidden
    layers of 4 .. 256 units (multiples of 4), Tanh or ReLU, no custom initialiser — None otherwise (and for
    the default torso, which the fused kernels serve).  Every other torso runs the same arithmetic as stock
    PyTorch-ROCm operators on the HBM-resident data (see `_StockTorch`).  The entries themselves take layers
    up to 384 units (tested per parameter tensor against float64 on (384, 260) ReLU and (256, 256) Tanh — the
    PPO / A2C entries in tests/test_gpu_layerwise_edges.py, the TRPO entries in tests/test_gpu_trpo_hip.py — and
    on the whole gradient vector on (384, 300) ReLU and (384, 8) Tanh for PPO / A2C, test_gpu_parity.py), but
    beyond 256 a layer is several 64-output slices each re-reading its input rows and rocBLAS wins — (384, 300) ReLU at N = 1 M: 41.4 ms vs 32.3 ms per learner iteration,
    profiles/r05_torso_timing.txt — so the agents hand such torsos to the stock operators
    (TONIC_AMD_TORSO_WIDE_HIP=1 keeps them on the HIP entries)."""
    import ctypes
    sizes = tuple(int(v) for v in torso.sizes)
    code = _TORSO_ACTIVATIONS.get(torso.activation)
    if fused_ppo_torso(torso) or code is None or not 1 <= len(sizes) <= 4:
        return None
    widest = 384 if os.environ.get('TONIC_AMD_TORSO_WIDE_HIP', '0') == '1' else 256
    if any(v < 4 or v > widest or v % 4 for v in sizes):
        return None
    if os.environ.get('TONIC_AMD_TORSO_STOCK', '0') == '1':      # (developer switch: A/B against stock torch)
        return None
    return len(sizes), (ctypes.c_int32 * len(sizes))(*sizes), code


class _StockTorch:
    """Networks outside the shapes of the hand-written kernels (tonic/torch/models/utils.py:4-23
    accepts any ``MLP(sizes, activation)``): forward, loss, autograd backward and the optimizer
    step are stock PyTorch-ROCm operators on the device-resident Segment / Buffer batches and on
    the very parameter views of the flat buffers — same data layout, same agent loops, same
    statistics rows as the fused path; still no CPU path (the agents refuse to initialise without
    a GPU).  Slower than the fused kernels and with one host read-back per step for the flags the
    fused path keeps on the device; pinned on goldens of the reference's agents with such torsos
    (tests/golden/ppo_relu256_small.npz, sac_uneven_small.npz)."""

    stock = False

    def _stock_setup(self, factory, default_lr):
        self.stock = True
        variables = [p for p in self.variables]
        for p in variables:
            p.requires_grad_(True)
        self.torch_optimizer = (factory(variables) if factory is not None
                                else torch.optim.Adam(variables, lr=default_lr))
        # the real torch scheduler on the real optimizer, stepped after each of its steps (`_stock_optimizer_step`)
        scheduler = getattr(self, 'lr_scheduler', None)
        self.torch_scheduler = scheduler(self.torch_optimizer) if scheduler is not None else None

    def _stock_optimizer_step(self):
        """optimizer.step(), scheduler.step(): torch's order, the step counts of the device path."""
        self.torch_optimizer.step()
        if self.torch_scheduler is not None:
            self.torch_scheduler.step()
        self.steps_enqueued += 1
        self.state[0] += 1

    def _stock_reduce(self):
        """Several ranks (equal shards): the per-rank mean gradients are averaged."""
        from tonic_amd import parallel
        if not parallel.exchanging():
            return
        world = parallel.world_size()
        for p in self.variables:
            if p.grad is not None:
                torch.distributed.all_reduce(p.grad)
                p.grad /= world

    def _stock_apply(self):
        self._stock_reduce()
        if self.gradient_clip > 0:
            torch.nn.utils.clip_grad_norm_(self.variables, self.gradient_clip)
        self._stock_optimizer_step()


class _FlatUpdater(_StockTorch):
    stats_kind = 0
    torso = None            # (layers, sizes, activation): the tonic_*_torso entries serve this network
    schedule = None         # the packed tonic_lr_schedule_t of `lr_scheduler=` (`_setup`); None: the rate is `lr`

    def _setup(self, flat, hyper):
        self.lib = _lib.load()
        self.flat = flat
        self.hyper = hyper
        device = flat.flat.device
        self.count = flat.count
        self.grad_sums = torch.zeros(self.count + INFO_WIDTH, dtype=torch.float32, device=device)
        self.plain = plain_adam(hyper)      # the pair launch and the fused off-policy iteration serve this rule only
        # ... scheduled or not: `schedule` is the packed tonic_lr_schedule_t of `lr_scheduler=`, None without one
        self.schedule = lr_schedule_rule(getattr(self, 'lr_scheduler', None), getattr(self, 'optimizer', None),
                                         hyper['lr'])
        self.optim = _OptimizerState(self.lib, hyper, self.count, device, self.schedule)
        self.rule, self.slots, self.state = self.optim.rule, self.optim.slots, self.optim.state
        self.exp_avg, self.exp_avg_sq = self.optim.exp_avg, self.optim.exp_avg_sq
        self.steps_enqueued = 0     # host mirror of state[0] (off-policy: every enqueued step is taken)
        self.workspace = None
        self.scratch_info = torch.zeros(INFO_WIDTH, dtype=torch.float32, device=device)
        self.gradient_clip = float(getattr(self, 'gradient_clip', 0) or 0)
        self.clip_workspace = torch.zeros(self.lib.tonic_clip_workspace_bytes(self.count),
                                          dtype=torch.uint8, device=device)
        # Workgroups of the fused grad launches (0 = the kernel's own width).  Part of the
        # updater's configuration, not of a call: the grouping of the float32 partial sums follows
        # it, so results are reproducible as long as it stays what it is (agents.PPO sets the
        # critic's once, from the worker count — whether or not its iterations then run under
        # the next rollout).
        self.max_workgroups = 0
        self.world_size = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.world_size = torch.distributed.get_world_size()

    def learning_rate(self, step=None):
        """The rate the next optimizer step will use (`step`: the rate of the step taken after that many steps)."""
        if self.stock and step is None:
            return float(self.torch_optimizer.param_groups[0]['lr'])
        return self.optim.learning_rate(step)

    def schedule_signature(self):
        """What a captured graph bakes in of the schedule (None without one)."""
        return self.schedule.signature() if self.schedule is not None else None

    def _workspace_for(self, n):
        """Scratch of the grad kernels: per-workgroup partial images for the fused kernels; for
        shapes beyond them (O > 32, A > 8: csrc/mlpwide.hip) also the activations of the
        layer-by-layer passes."""
        actor = self.stats_kind == 1
        shape = (n, self.observation_size, self.action_size if actor else 1, 1 if actor else 0)
        if self.torso is not None:
            need = self.lib.tonic_ppo_torso_workspace_bytes(*shape, *self.torso[:2])
        else:
            need = self.lib.tonic_ppo_workspace_bytes(*shape)
        if need < 0:
            raise NotImplementedError(
                f'PPO networks with {self.observation_size} observations / '
                f'{getattr(self, "action_size", 1)} actions are outside the HIP kernels '
                '(O <= 384, A <= 32)')
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.grad_sums.device)
        return self.workspace

    def share_gradient_buffer(self, buffer):
        """Makes `grad_sums` a view of a caller-owned buffer so that several updaters' gradient
        sums travel in ONE all-reduce (the caller then passes allreduce=False to enqueue)."""
        assert buffer.numel() == self.count + INFO_WIDTH
        self.grad_sums = buffer

    def enqueue_clip(self, n_global, skip=None):
        """clip_grad_norm_ between backward and the optimizer step (actors.py:96-98,
        critics.py:24-25): on the (all-reduced) gradient sums, in place."""
        if self.gradient_clip > 0:
            _lib.check(self.lib.tonic_clip_grad_norm(
                _lib.ptr(self.grad_sums), self.count, 1.0 / n_global, self.gradient_clip, skip,
                _lib.ptr(self.clip_workspace), self.clip_workspace.numel(),
                _lib.current_stream()), 'tonic_clip_grad_norm')

    def _step(self, n_global, info_row, adv_stats=None, skip=None, kl_threshold=0.0,
              entropy_coeff=0.0, allreduce=True, targets=None):
        """All-reduce of the gradient sums (world > 1) + optimizer step + statistics.  `targets` =
        (flat target buffer, flat online buffer, offset of this block in them, coeff): the
        polyak update of ALL targets rides in the same launch (update_targets right after the
        step, as ddpg.py:105-112 orders them)."""
        from tonic_amd import parallel
        self.steps_enqueued += 1
        if parallel.exchanging() and allreduce:
            one_shot = parallel.one_shot(self.count + INFO_WIDTH)
            if one_shot is not None:
                one_shot.all_reduce(self.grad_sums)              # tonic_allreduce_f32
            else:
                torch.distributed.all_reduce(self.grad_sums)     # RCCL sum over xGMI
        self.enqueue_clip(n_global, skip)
        self.optim.enqueue(self.flat.flat, self.grad_sums, 1.0 / n_global, info_row, self.stats_kind, kl_threshold,
                           entropy_coeff, adv_stats, skip, targets)


def adam_step_constants(hyper, step):
    """{step_size, bias_correction2_sqrt} of optimizer step `step` (1-based) as float32 of the
    float64 values torch.optim.Adam forms in Python (adam.py:530-536)."""
    beta1, beta2 = hyper['betas']
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return hyper['lr'] / bias_correction1, bias_correction2 ** 0.5


def enqueue_step_pair(actor, critic, n_local, adv_stats, actor_info, critic_info):
    """The optimizer steps of a PPO iteration (ppo.py:33-46: actor, then critic) as ONE launch
    pair.  The gradient sums are final (all-reduced by the caller when world > 1)."""
    ha, hc = actor.hyper, critic.hyper
    if actor.stock or critic.stock or not (actor.plain and critic.plain) or \
            (ha['betas'], ha['eps']) != (hc['betas'], hc['eps']):                            # separately
        actor.enqueue_step(n_local, adv_stats, actor_info, allreduce=False)
        critic.enqueue_step(n_local, critic_info, allreduce=False)
        return
    n_global = n_local * actor.world_size
    actor.enqueue_clip(n_global, actor.stop_flag_ptr())
    critic.enqueue_clip(n_global)
    p = _lib.ptr
    # (`plain` is the rule; a schedule on either network keeps the ONE launch, through the scheduled pair)
    entry, schedules = 'tonic_adam_step_pair', ()
    if actor.schedule is not None or critic.schedule is not None:
        entry = 'tonic_scheduled_adam_step_pair'
        schedules = tuple(ctypes.byref(u.schedule) if u.schedule is not None else None for u in (actor, critic))
    _lib.check(getattr(actor.lib, entry)(
        p(actor.flat.flat), p(actor.grad_sums), p(actor.exp_avg), p(actor.exp_avg_sq),
        p(actor.state), actor.count, ha['lr'], actor.stats_kind, float(actor.kl_threshold),
        float(actor.entropy_coeff), p(adv_stats), p(actor_info), actor.stop_flag_ptr(),
        p(critic.flat.flat), p(critic.grad_sums), p(critic.exp_avg), p(critic.exp_avg_sq),
        p(critic.state), critic.count, hc['lr'], critic.stats_kind, p(critic_info),
        1.0 / (n_local * actor.world_size), ha['betas'][0], ha['betas'][1], ha['eps'], *schedules,
        _lib.current_stream()), entry)


class ClippedRatio(_FlatUpdater):
    stats_kind = 1

    def __init__(self, optimizer=None, ratio_clip=0.2, kl_threshold=0.015, entropy_coeff=0,
                 gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.optimizer = optimizer
        self.ratio_clip = ratio_clip
        self.kl_threshold = kl_threshold
        self.entropy_coeff = entropy_coeff
        self.gradient_clip = gradient_clip

    def initialize(self, model):
        self.model = model
        self._setup(model.flat_actor, optimizer_hyperparameters(self.optimizer, 3e-4))
        self.variables = model.flat_actor.params
        self.observation_size = model.actor.torso.model[0].in_features
        self.action_size = model.actor.head.log_scale.shape[1]
        if not fused_ppo_torso(model.actor.torso):
            self.torso = hip_ppo_torso(model.actor.torso)
            if self.torso is None or self.lib.tonic_ppo_torso_param_count(
                    self.observation_size, self.action_size, 1, self.torso[0], self.torso[1]) != self.count:
                self.torso = None
                self._stock_setup(self.optimizer, 3e-4)

    def _stock_grad(self, observations, actions, advantages, adv_stats, log_probs):
        """actors.py:70-112 up to the optimizer step (ClippedRatio; ratio_clip < 0: the plain
        policy gradient of actors.py:22-51).  `advantages` are raw: normalised here with the
        segment's statistics like `get_full` does (segments.py:41-46)."""
        self._stock_row = None
        if int(self.state[1]) != 0:                      # stopped earlier in this update
            return
        mean, std, all_zero, normalise = (float(v) for v in adv_stats.tolist())
        if normalise:
            advantages = (advantages - mean) / std
        zero = torch.zeros((), device=observations.device)
        if all_zero:                                      # actors.py:71-75 / 23-26
            with torch.no_grad():
                distributions = self.model.actor(observations)
                self._stock_row = (zero, zero, distributions.entropy().mean(), zero,
                                   distributions.stddev.mean(), False)
            return
        self.torch_optimizer.zero_grad()
        distributions = self.model.actor(observations)
        new_log_probs = distributions.log_prob(actions).sum(dim=-1)
        entropy = distributions.entropy().mean()
        if self.ratio_clip >= 0:
            ratios_1 = torch.exp(new_log_probs - log_probs)
            surrogates_1 = advantages * ratios_1
            ratios_2 = torch.clamp(ratios_1, 1 - self.ratio_clip, 1 + self.ratio_clip)
            loss = -torch.min(surrogates_1, advantages * ratios_2).mean()
        else:
            loss = -(advantages * new_log_probs).mean()
        if self.entropy_coeff != 0:
            loss = loss - self.entropy_coeff * entropy
        loss.backward()
        with torch.no_grad():
            kl = (log_probs - new_log_probs).mean()
            if self.ratio_clip >= 0:
                clipped = ratios_1.gt(1 + self.ratio_clip) | ratios_1.lt(1 - self.ratio_clip)
                clip_fraction = clipped.float().mean()
            else:
                clip_fraction = zero
            self._stock_row = (loss.detach(), kl, entropy.detach(), clip_fraction,
                               distributions.stddev.mean().detach(), True)

    def _stock_step(self, info_row):
        if self._stock_row is None:
            return
        loss, kl, entropy, clip_fraction, std, step = self._stock_row
        if step:
            self._stock_apply()
        stop = bool(kl > self.kl_threshold)               # actors.py:112
        info_row[:5] = torch.stack([loss, kl, entropy, clip_fraction, std])
        info_row[5] = float(stop)
        info_row[6] = 1.0
        if stop:
            self.state[1] = 1

    def stop_flag_ptr(self):
        return self.state.data_ptr() + 4

    def reset_stop(self):
        self.state[1:2].zero_()

    def enqueue_grad(self, observations, actions, advantages, adv_stats, log_probs):
        if self.stock:
            return self._stock_grad(observations, actions, advantages, adv_stats, log_probs)
        n = observations.shape[0]
        ws = self._workspace_for(n)
        p = _lib.ptr
        if self.torso is not None:
            _lib.check(self.lib.tonic_ppo_actor_grad_torso(
                *self.torso, p(self.flat.flat), p(observations), p(actions), p(advantages), p(adv_stats),
                p(log_probs), p(self.grad_sums), n, self.observation_size, self.action_size,
                float(self.ratio_clip), float(self.entropy_coeff), self.stop_flag_ptr(),
                p(ws), ws.numel(), _lib.current_stream()), 'tonic_ppo_actor_grad_torso')
            return
        _lib.check(self.lib.tonic_ppo_actor_grad(
            p(self.flat.flat), p(observations), p(actions), p(advantages), p(adv_stats),
            p(log_probs), p(self.grad_sums), n, self.observation_size, self.action_size,
            float(self.ratio_clip), float(self.entropy_coeff), self.stop_flag_ptr(),
            self.max_workgroups, p(ws), ws.numel(), _lib.current_stream()), 'tonic_ppo_actor_grad')

    def enqueue_step(self, n_local, adv_stats, info_row, allreduce=True):
        if self.stock:
            return self._stock_step(info_row)
        self._step(n_local * self.world_size, info_row, adv_stats, self.stop_flag_ptr(),
                   self.kl_threshold, self.entropy_coeff, allreduce)

    def enqueue(self, observations, actions, advantages, adv_stats, log_probs, info_row):
        self.enqueue_grad(observations, actions, advantages, adv_stats, log_probs)
        self.enqueue_step(observations.shape[0], adv_stats, info_row)

    def __call__(self, observations, actions, advantages, log_probs):
        """Drop-in form (actors.py:70-112): `advantages` are final (already normalised)."""
        all_zero = bool((advantages == 0).all())
        adv_stats = torch.tensor([0., 1., float(all_zero), 0.], device=advantages.device)
        self.reset_stop()
        self.scratch_info.zero_()
        self.enqueue(observations, actions, advantages, adv_stats, log_probs, self.scratch_info)
        row = self.scratch_info.cpu()
        self.reset_stop()
        out = {k: row[i].clone() for i, k in enumerate(ACTOR_INFO)}
        out['stop'] = out['stop'] > 0.5
        return out


class StochasticPolicyGradient(ClippedRatio):
    """actors.py:9-51 (A2C): loss = -mean(advantages * log_probs) [- entropy_coeff * entropy], one
    Adam step.  Same fused kernel as ClippedRatio in its plain mode (`ratio_clip < 0` in the C ABI:
    the gradient of -adv * logp is -adv, nothing to clip) and no KL stop."""

    def __init__(self, optimizer=None, entropy_coeff=0, gradient_clip=0, lr_scheduler=None):
        super().__init__(optimizer=optimizer, ratio_clip=-1.0, kl_threshold=float('inf'),
                         entropy_coeff=entropy_coeff, gradient_clip=gradient_clip, lr_scheduler=lr_scheduler)

    def __call__(self, observations, actions, advantages, log_probs):
        out = super().__call__(observations, actions, advantages, log_probs)
        return {k: out[k] for k in ('loss', 'kl', 'entropy', 'std')}


class ConjugateGradient:
    """optimizers.py:25-115 — truncated natural gradient with a backtracking line search, on the
    device: the search direction solves H x = g by `conjugate_gradient_steps` CG iterations whose
    Hessian-vector products are autograd double-backward passes of the constraint (KL) over the
    HBM-resident batch; then x is scaled to the trust region and shrunk until the constraint holds
    and the loss did not rise.  The CG scalars stay 0-dim device tensors (no host sync inside the
    loop); each backtracking trial reads two scalars back, like the reference.

    Several ranks (equal shards of the batch): the loss / constraint values, the gradient and every
    Hessian-vector product are batch MEANS, so each is averaged over the ranks with one all-reduce
    and all ranks walk through identical CG iterations and backtracking trials."""

    def __init__(self, conjugate_gradient_steps=10, damping_coefficient=0.1,
                 constraint_threshold=0.01, backtrack_steps=10, backtrack_coefficient=0.8):
        self.conjugate_gradient_steps = conjugate_gradient_steps
        self.damping_coefficient = damping_coefficient
        self.constraint_threshold = constraint_threshold
        self.backtrack_steps = backtrack_steps
        self.backtrack_coefficient = backtrack_coefficient

    def optimize(self, loss_function, constraint_function, variables):
        from tonic_amd import parallel
        eps = 1e-8                                              # optimizers.py:5
        world = parallel.world_size() if parallel.exchanging() else 1

        def across(tensor):
            """Mean over the ranks of a per-rank batch mean (in place; one rank: nothing)."""
            if world > 1:
                torch.distributed.all_reduce(tensor)
                tensor /= world
            return tensor

        def flat(tensors):
            return torch.cat([t.reshape(-1) for t in tensors])

        def hessian_vector(x):                                  # optimizers.py:36-48
            first = flat(torch.autograd.grad(constraint_function(), variables, create_graph=True))
            second = across(flat(torch.autograd.grad((first * x).sum(), variables)))
            if self.damping_coefficient > 0:
                second = second + self.damping_coefficient * x
            return second

        def assign(values):                                     # optimizers.py:13-22
            offset = 0
            with torch.no_grad():
                for v in variables:
                    v.copy_(values[offset:offset + v.numel()].view(v.shape))
                    offset += v.numel()

        def trial(scale):                                       # optimizers.py:68-74
            assign(start - alpha * direction * scale)
            with torch.no_grad():
                both = across(torch.stack([constraint_function(), loss_function()]))
                return both[0], both[1]

        start = flat([v.detach() for v in variables]).clone()
        loss = loss_function()
        gradient = across(flat(torch.autograd.grad(loss, variables)))
        start_loss = float(across(loss.detach().clone()))
        zero = torch.zeros((), dtype=torch.float32)
        residual_dot = gradient.dot(gradient)
        if float(residual_dot) == 0:                            # optimizers.py:55-56, 87-91
            return zero, zero, torch.as_tensor(0, dtype=torch.int32)
        direction = torch.zeros_like(gradient)
        residual, search = gradient.clone(), gradient.clone()
        for _ in range(self.conjugate_gradient_steps):          # optimizers.py:58-65
            z = hessian_vector(search)
            step = residual_dot / (search.dot(z) + eps)
            direction += step * search
            residual -= step * z
            new_dot = residual.dot(residual)
            search = residual + (new_dot / residual_dot) * search
            residual_dot = new_dot
        alpha = torch.sqrt(2 * self.constraint_threshold /
                           direction.dot(hessian_vector(direction)) + eps)      # optimizers.py:93-94
        if self.backtrack_steps is None or self.backtrack_coefficient is None:
            constraint, loss = trial(1)
            return constraint.cpu(), loss.cpu()
        for i in range(self.backtrack_steps):                   # optimizers.py:101-113
            constraint, loss = trial(self.backtrack_coefficient ** i)
            if float(constraint) <= self.constraint_threshold and float(loss) <= start_loss:
                break
            if i == self.backtrack_steps - 1:
                constraint, loss = trial(0)
                i = self.backtrack_steps
        return constraint.cpu(), loss.cpu(), torch.as_tensor(i + 1, dtype=torch.int32)

    def optimize_flat(self, parameters, loss_gradient, fisher_vector, evaluate):
        """The same step — same `eps`, recurrences, step length, backtracking rule and `trial(0)` fallback as
        `optimize`, line for line — for a caller that evaluates the batch itself (TrustRegionPolicyGradient's
        HIP kernels) on ONE flat parameter vector instead of a list of views:

            loss_gradient()   -> (gradient [P], loss), batch means over all ranks, at `parameters`
            fisher_vector(x)  -> H x [P] without the damping term, a batch mean over all ranks
            evaluate()        -> tensor {constraint, loss} at what `parameters` holds now

        `parameters` is moved in place to the accepted trial, as `optimize` leaves its variables."""
        eps = 1e-8                                              # optimizers.py:5

        def hessian_vector(x):                                  # optimizers.py:36-48
            second = fisher_vector(x)
            if self.damping_coefficient > 0:
                second = second + self.damping_coefficient * x
            return second

        def trial(scale):                                       # optimizers.py:68-74
            parameters.copy_(start - alpha * direction * scale)
            both = evaluate()
            return both[0], both[1]

        start = parameters.detach().clone()
        gradient, loss = loss_gradient()
        start_loss = float(loss)
        zero = torch.zeros((), dtype=torch.float32)
        residual_dot = gradient.dot(gradient)
        if float(residual_dot) == 0:                            # optimizers.py:55-56, 87-91
            return zero, zero, torch.as_tensor(0, dtype=torch.int32)
        direction = torch.zeros_like(gradient)
        residual, search = gradient.clone(), gradient.clone()
        for _ in range(self.conjugate_gradient_steps):          # optimizers.py:58-65
            z = hessian_vector(search)
            step = residual_dot / (search.dot(z) + eps)
            direction += step * search
            residual -= step * z
            new_dot = residual.dot(residual)
            search = residual + (new_dot / residual_dot) * search
            residual_dot = new_dot
        alpha = torch.sqrt(2 * self.constraint_threshold /
                           direction.dot(hessian_vector(direction)) + eps)      # optimizers.py:93-94
        if self.backtrack_steps is None or self.backtrack_coefficient is None:
            constraint, loss = trial(1)
            return constraint.cpu(), loss.cpu()
        for i in range(self.backtrack_steps):                   # optimizers.py:101-113
            constraint, loss = trial(self.backtrack_coefficient ** i)
            if float(constraint) <= self.constraint_threshold and float(loss) <= start_loss:
                break
            if i == self.backtrack_steps - 1:
                constraint, loss = trial(0)
                i = self.backtrack_steps
        return constraint.cpu(), loss.cpu(), torch.as_tensor(i + 1, dtype=torch.int32)


class TrustRegionPolicyGradient:
    """actors.py:115-156 (TRPO): the truncated natural-gradient step of `ConjugateGradient` on the
    HBM-resident Segment.  `locs` / `scales` of the behaviour policy may be omitted: the parameters have not
    moved since the rollout, so the actor itself reproduces them.

    HIP path (csrc/trpo_body.h, the tonic_trpo_* entries; `self.hip` after `initialize`): the loss gradient,
    the Fisher-vector products and the line-search trials are kernels over the batch.  The parameters do
    not move during the conjugate-gradient loop, so ONE forward pass per update leaves the activations in
    the workspace and every product reuses them; with the behaviour policy this network's own output the
    Hessian of the KL is the Gauss-Newton product J^T M J v the kernels form.  Taken for an
    `MLP(sizes, activation)` torso the layer-by-layer kernels serve (the default one included), a
    `DetachedScaleGaussianPolicyHead` as the reference builds it (Tanh locations, Normal, scales clamped to
    [1e-4, 1]) and a `ConjugateGradient` optimizer, when the behaviour policy is not passed in.

    Stock path, exactly as before: every other network or optimizer, explicit `locs` / `scales` (Gauss-Newton
    is then not the Hessian), or TONIC_AMD_TRPO_HIP=0 — the loss, the KL and the products are PyTorch autograd
    over `model.actor`, whose parameters ARE views of the flat HBM buffer the act kernels read."""

    def __init__(self, optimizer=None, entropy_coeff=0):
        self.optimizer = optimizer or ConjugateGradient()
        self.entropy_coeff = entropy_coeff

    def initialize(self, model):
        self.model = model
        self.variables = list(model.flat_actor.params)
        self.world_size = 1
        self.hip_workspace = None
        served = self._served_torso(model)                      # decided once; None: the stock path
        self.hip, self.hip_torso = served is not None, None
        if self.hip:
            self.lib = _lib.load()
            self.hip_torso, self.observation_size, self.action_size = served

    def _served_torso(self, model):
        """((layers, sizes, activation) for the tonic_trpo_* entries, O, A), or None."""
        import ctypes
        from tonic_amd.torch import models
        if os.environ.get('TONIC_AMD_TRPO_HIP', '1') == '0':
            return None
        actor, flat = model.actor, model.flat_actor
        torso, head = getattr(actor, 'torso', None), getattr(actor, 'head', None)
        if not isinstance(self.optimizer, ConjugateGradient) or not flat.flat.is_cuda:
            return None
        if type(getattr(actor, 'encoder', None)) is not models.ObservationEncoder or \
                actor.encoder.observation_normalizer or not isinstance(torso, models.MLP):
            return None
        if type(head) is not models.DetachedScaleGaussianPolicyHead or head.loc_activation is not torch.nn.Tanh \
                or head.loc_fn is not None or head.distribution is not torch.distributions.normal.Normal \
                or (head.scale_min, head.scale_max) != (1e-4, 1.):
            return None                      # (the kernels clamp the scales to the reference's defaults, actors.py:39-40)
        if fused_ppo_torso(torso):
            served = 2, (ctypes.c_int32 * 2)(64, 64), 1
        else:
            served = hip_ppo_torso(torso)
            if served is None:
                return None
        lib = _lib.load()
        O, A = torso.model[0].in_features, head.log_scale.shape[1]
        if lib.tonic_ppo_torso_param_count(O, A, 1, served[0], served[1]) != flat.count:
            return None
        if lib.tonic_trpo_workspace_bytes(1, O, A, served[0], served[1]) < 0:
            return None
        return served, O, A

    def _hip_workspace_for(self, n):
        need = self.lib.tonic_trpo_workspace_bytes(n, self.observation_size, self.action_size,
                                                   self.hip_torso[0], self.hip_torso[1])
        if self.hip_workspace is None or self.hip_workspace.numel() < need:
            self.hip_workspace = torch.empty(need, dtype=torch.uint8, device=self.model.flat_actor.flat.device)
        return self.hip_workspace

    def __call__(self, observations, actions, log_probs, advantages, locs=None, scales=None):
        from tonic_amd import parallel
        device = self.variables[0].device
        observations, actions, log_probs, advantages = (
            torch.as_tensor(v, dtype=torch.float32, device=device)
            for v in (observations, actions, log_probs, advantages))
        hip = self.hip and locs is None and scales is None
        if hip:
            pass                                               # (tonic_trpo_prepare forms them)
        elif locs is None or scales is None:
            with torch.no_grad():
                behaviour = self.model.actor(observations)
                locs, scales = behaviour.loc, behaviour.stddev
        else:
            locs, scales = (torch.as_tensor(v, dtype=torch.float32, device=device)
                            for v in (locs, scales))
        nothing = (advantages == 0.).all().float()             # actors.py:127-130 (on ALL ranks)
        if parallel.exchanging():
            torch.distributed.all_reduce(nothing, op=torch.distributed.ReduceOp.MIN)
        if bool(nothing):
            zero = torch.zeros((), dtype=torch.float32)
            return dict(loss=zero, kl=zero, backtrack_steps=torch.as_tensor(0, dtype=torch.int32))
        if hip:
            kl, loss, steps = self._hip_optimize(observations, actions, log_probs, advantages)
            return dict(loss=loss, kl=kl, backtrack_steps=steps)
        kl, loss, steps = self.optimizer.optimize(
            loss_function=lambda: self._loss(observations, actions, log_probs, advantages),
            constraint_function=lambda: self._kl(observations, locs, scales),
            variables=self.variables)
        return dict(loss=loss, kl=kl, backtrack_steps=steps)

    def _hip_optimize(self, observations, actions, log_probs, advantages):
        """`ConjugateGradient.optimize_flat` over the tonic_trpo_* entries.  The entries return SUMS over this
        rank's rows; they become batch means here (/ n_local; the KL and its products / (n_local * A)) and
        means over the ranks through the same `across` as the stock path."""
        from tonic_amd import parallel
        lib, p, stream = self.lib, _lib.ptr, _lib.current_stream()
        flat = self.model.flat_actor.flat
        P, O, A = flat.numel(), self.observation_size, self.action_size
        observations, actions, log_probs, advantages = (
            v.contiguous() for v in (observations, actions, log_probs, advantages))
        n = observations.shape[0]
        ws = self._hip_workspace_for(n)
        shape, scratch = (n, O, A), (p(ws), ws.numel(), stream)
        batch = (p(observations), p(actions), p(advantages), p(log_probs))
        coeff = float(self.entropy_coeff)
        world = parallel.world_size() if parallel.exchanging() else 1

        def across(tensor):
            if world > 1:
                torch.distributed.all_reduce(tensor)
                tensor /= world
            return tensor

        _lib.check(lib.tonic_trpo_prepare(*self.hip_torso, p(flat), p(observations), *shape, None, None,
                                          *scratch), 'tonic_trpo_prepare')

        def loss_gradient():
            sums = torch.empty(P + INFO_WIDTH, dtype=torch.float32, device=flat.device)
            _lib.check(lib.tonic_trpo_loss_grad(*self.hip_torso, p(flat), *batch, p(sums), *shape, coeff,
                                                *scratch), 'tonic_trpo_loss_grad')
            loss = sums[P] / n
            if coeff != 0:
                loss = loss - coeff * (sums[P + 3] / n)         # actors.py:148-149 (slot 3: n * entropy)
            return across(sums[:P] / n), across(loss.clone())

        def fisher_vector(x):
            x = x.contiguous()
            sums = torch.empty(P + INFO_WIDTH, dtype=torch.float32, device=flat.device)
            _lib.check(lib.tonic_trpo_fisher_vector(*self.hip_torso, p(flat), p(observations), p(x), p(sums),
                                                    *shape, *scratch), 'tonic_trpo_fisher_vector')
            return across(sums[:P] / (n * A))

        def evaluate():
            out = torch.empty(2, dtype=torch.float32, device=flat.device)
            _lib.check(lib.tonic_trpo_evaluate(*self.hip_torso, p(flat), *batch, *shape, coeff, p(out),
                                               *scratch), 'tonic_trpo_evaluate')
            return across(torch.stack([out[1] / (n * A), out[0] / n]))

        return self.optimizer.optimize_flat(flat, loss_gradient, fisher_vector, evaluate)

    def _loss(self, observations, actions, old_log_probs, advantages):        # actors.py:142-150
        distributions = self.model.actor(observations)
        log_probs = distributions.log_prob(actions).sum(dim=-1)
        loss = -(torch.exp(log_probs - old_log_probs) * advantages).mean()
        if self.entropy_coeff != 0:
            loss = loss - self.entropy_coeff * distributions.entropy().mean()
        return loss

    def _kl(self, observations, locs, scales):                                # actors.py:152-156
        distributions = self.model.actor(observations)
        behaviour = type(distributions)(locs, scales)
        return torch.distributions.kl.kl_divergence(distributions, behaviour).mean()


class VRegression(_FlatUpdater):
    stats_kind = 2

    def __init__(self, loss=None, optimizer=None, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        if loss is not None and not isinstance(loss, torch.nn.MSELoss):
            raise NotImplementedError('only the default MSE loss is fused')
        self.loss = loss
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip

    def initialize(self, model):
        self.model = model
        self._setup(model.flat_critic, optimizer_hyperparameters(self.optimizer, 1e-3))
        self.variables = model.flat_critic.params
        self.observation_size = model.critic.torso.model[0].in_features
        self.normalizer = model.observation_normalizer
        # the Return normaliser of the value head (critics.py:17-19): the *_ranged entries squash with its
        # _low / _high (stock torch applies it through model.critic)
        self.return_normalizer = getattr(model.critic.head, 'return_normalizer', None) or None
        if not fused_ppo_torso(model.critic.torso):
            self.torso = hip_ppo_torso(model.critic.torso)
            if self.torso is None or self.lib.tonic_ppo_torso_param_count(
                    self.observation_size, 1, 0, self.torso[0], self.torso[1]) != self.count:
                self.torso = None
                self._stock_setup(self.optimizer, 1e-3)
        if self.normalizer is None:
            device = self.grad_sums.device
            self._unit_mean = torch.zeros(self.observation_size, device=device)
            self._unit_std = torch.ones(self.observation_size, device=device)

    def norm_tensors(self):
        if self.normalizer is None:
            return self._unit_mean, self._unit_std
        return self.normalizer._mean.data, self.normalizer._std.data

    def norm_clip(self):
        """MeanStd(clip=...) (mean_stds.py:37-38) as the C ABI wants it: 0 = None."""
        return float(getattr(self.normalizer, 'clip', None) or 0.0)

    def range_tensors(self):
        """The Return normaliser's (_low, _high) on the device, or None without one."""
        if self.return_normalizer is None:
            return None
        return self.return_normalizer._low.data, self.return_normalizer._high.data

    def forward_values(self, observations, out):
        if self.stock:
            with torch.no_grad():
                out.copy_(self.model.critic(observations))
            return out
        mean, std = self.norm_tensors()
        p = _lib.ptr
        n = observations.shape[0]
        ws = self._workspace_for(n)
        low, high = map(p, self.range_tensors() or (None, None))         # both NULL: the plain head
        prefix, name = ((), 'tonic_value_forward_wide_ranged') if self.torso is None else \
            (self.torso, 'tonic_value_forward_torso_ranged')
        _lib.check(getattr(self.lib, name)(
            *prefix, p(self.flat.flat), p(mean), p(std), self.norm_clip(), p(observations), p(out), n,
            self.observation_size, p(ws), ws.numel(), low, high, _lib.current_stream()), name)
        return out

    def enqueue_grad(self, observations, returns, norm=None, value_range=None):
        """`norm`: (mean, std) to use instead of the normaliser's tensors — a snapshot, for
        iterations that run while the normaliser is being updated (agents.PPO._update); `value_range`:
        the same for the Return normaliser's (low, high)."""
        if self.stock:                                    # critics.py:18-28
            self.torch_optimizer.zero_grad()
            values = self.model.critic(observations)
            loss = torch.nn.functional.mse_loss(values, returns)
            loss.backward()
            self._stock_row = (loss.detach(), values.detach().mean())
            return
        n = observations.shape[0]
        ws = self._workspace_for(n)
        mean, std = norm if norm is not None else self.norm_tensors()
        p = _lib.ptr
        low, high = map(p, value_range or self.range_tensors() or (None, None))   # both NULL: the plain head
        if self.torso is not None:
            _lib.check(self.lib.tonic_value_regression_grad_torso_ranged(
                *self.torso, p(self.flat.flat), p(mean), p(std), self.norm_clip(), p(observations),
                p(returns), p(self.grad_sums), n, self.observation_size, p(ws), ws.numel(), low, high,
                _lib.current_stream()), 'tonic_value_regression_grad_torso_ranged')
            return
        _lib.check(self.lib.tonic_value_regression_grad_ranged(
            p(self.flat.flat), p(mean), p(std), self.norm_clip(), p(observations), p(returns),
            p(self.grad_sums), n, self.observation_size, self.max_workgroups, p(ws), ws.numel(),
            low, high, _lib.current_stream()), 'tonic_value_regression_grad_ranged')

    def enqueue_step(self, n_local, info_row, allreduce=True):
        if self.stock:
            self._stock_apply()
            info_row[:2] = torch.stack(self._stock_row)
            info_row[6] = 1.0
            return
        self._step(n_local * self.world_size, info_row, allreduce=allreduce)

    def enqueue(self, observations, returns, info_row):
        self.enqueue_grad(observations, returns)
        self.enqueue_step(observations.shape[0], info_row)

    def __call__(self, observations, returns):
        """Drop-in form (critics.py:18-28).  `v` is the pre-step value vector."""
        values = torch.empty(observations.shape[0], device=observations.device)
        self.forward_values(observations, values)
        self.scratch_info.zero_()
        self.enqueue(observations, returns, self.scratch_info)
        row = self.scratch_info.cpu()
        return dict(loss=row[0].clone(), v=values.cpu())


# ----------------------------------------------------------------- off-policy (SAC / TD3)

_Q_ACTIVATIONS = {torch.nn.ReLU: 1, torch.nn.Tanh: 2, torch.nn.ELU: 3}       # GemmAct of csrc/gemm16.h


def _torso_width(torso, generic=False):
    """The `H` argument of the off-policy entries: the width of the reference's torso — two ReLU layers of one
    width, which the fused kernels hold (csrc/mlpfwd.hip) — or tonic_mlp_torso(layers, sizes, activation) for any
    other torso of 1 .. 4 layers of 1 .. 4095 units with ReLU / Tanh / ELU (unequal widths: the (400, 300) class;
    deeper or shallower torsos), which every off-policy entry runs layer by layer on gemm16 launches.  `generic`:
    the caller has a stock-torch form, which TONIC_AMD_TORSO_STOCK=1 selects for such torsos.  Anything else
    raises (callers with a stock-torch form catch it)."""
    sizes = tuple(int(v) for v in torso.sizes)
    plain = len(sizes) == 2 and sizes[0] == sizes[1] and torso.activation is torch.nn.ReLU
    if plain:                              # (a plain width goes through the C ABI's `H` as is)
        return sizes[0]
    code = _Q_ACTIVATIONS.get(torso.activation)
    to_stock = generic and os.environ.get('TONIC_AMD_TORSO_STOCK', '0') == '1'
    if code is not None and 1 <= len(sizes) <= 4 and all(1 <= v <= 4095 for v in sizes) and not to_stock:
        import ctypes
        packed = _lib.load().tonic_mlp_torso(len(sizes), (ctypes.c_int32 * len(sizes))(*sizes), code)
        if packed > 0:
            return packed
    raise NotImplementedError('the off-policy kernels serve torsos of 1 .. 4 layers of 1 .. 4095 units with ReLU / '
                              'Tanh / ELU, the same for actor and critic (SAC, TD3 and DDPG run any other torso on '
                              f'stock torch operators), got {sizes} / {torso.activation}')


_DEFAULT_SCALE_BOUNDS = (np.float32(1e-4), np.float32(1.))        # actors.py:39-40, 71-72, as the kernels hold them

# what the kernels of each family compute at the policy's head (the initialisers and log_scale_init stay free)
_HEAD_RULES = {
    'sac': ('GaussianPolicyHead', dict(loc_activation='Identity', scale_activation='Softplus',
                                       distribution='SquashedMultivariateNormalDiag'), 'any'),
    'mpo': ('GaussianPolicyHead', dict(loc_activation='Tanh', scale_activation='Softplus', distribution='Normal'),
            'any'),
    'deterministic': ('DeterministicPolicyHead', dict(activation='Tanh'), None),
    'on_policy': ('DetachedScaleGaussianPolicyHead', dict(loc_activation='Tanh', distribution='Normal'), 'default'),
}


def policy_head_rule(head, family):
    """What the HIP kernels of `family` ('sac', 'mpo', 'deterministic', 'on_policy') compute for this policy head, or
    NotImplementedError naming the argument they do not serve (no device needed).  Served:
      sac            GaussianPolicyHead(loc_activation=Identity, scale_activation=Softplus,
                     distribution=SquashedMultivariateNormalDiag), any 0 < scale_min <= scale_max
      mpo            GaussianPolicyHead(loc_activation=Tanh, scale_activation=Softplus, distribution=Normal), any bounds
      deterministic  DeterministicPolicyHead(activation=Tanh)                                  (DDPG, TD3, D4PG)
      on_policy      DetachedScaleGaussianPolicyHead(loc_activation=Tanh, distribution=Normal) with the default
                     scale_min=1e-4, scale_max=1: the PPO / A2C / TRPO kernels hold those bounds
    Returns the scale's (scale_min, scale_max) as the float32 the kernels clamp to; None for a deterministic head."""
    from tonic_amd.torch import models
    class_name, arguments, bounds = _HEAD_RULES[family]
    served = f'{class_name}(' + ', '.join(f'{k}={v}' for k, v in arguments.items()) + ')' + \
        {None: '', 'any': ' with any 0 < scale_min <= scale_max',
         'default': ' with the default scale_min=1e-4, scale_max=1'}[bounds]

    def refuse(argument, value):
        raise NotImplementedError(f'the {family} kernels serve {served}; got {argument}={value!r}')

    if type(head) is not getattr(models, class_name):       # (a subclass may compute anything in its forward)
        refuse('head', type(head).__name__)
    wanted = dict(Identity=torch.nn.Identity, Softplus=torch.nn.Softplus, Tanh=torch.nn.Tanh,
                  Normal=torch.distributions.normal.Normal,
                  SquashedMultivariateNormalDiag=models.SquashedMultivariateNormalDiag)
    for argument, name in arguments.items():
        if getattr(head, argument) is not wanted[name]:
            refuse(argument, getattr(head, argument))
    if bounds is None:
        return None
    low, high = np.float32(head.scale_min), np.float32(head.scale_max)
    if not (0 < low and np.isfinite(low)):
        refuse('scale_min', head.scale_min)
    if not (low <= high and np.isfinite(high)):
        refuse('scale_max', head.scale_max)
    if bounds == 'default' and (low, high) != _DEFAULT_SCALE_BOUNDS:
        refuse('scale_min' if low != _DEFAULT_SCALE_BOUNDS[0] else 'scale_max',
               head.scale_min if low != _DEFAULT_SCALE_BOUNDS[0] else head.scale_max)
    return low, high


def _actor_code(torso, bounds, generic=False):
    """The `H` argument wherever an entry runs the actor: the torso's own code (`_torso_width`), or — a Gaussian head
    with bounds other than the defaults — the code tonic_mlp_torso_head registers for torso + bounds."""
    code = _torso_width(torso, generic)
    if bounds is None or tuple(bounds) == _DEFAULT_SCALE_BOUNDS:
        return code
    sizes = tuple(int(v) for v in torso.sizes)
    lib = _lib.load()
    code = lib.tonic_mlp_torso_head(len(sizes), (ctypes.c_int32 * len(sizes))(*sizes),
                                    _Q_ACTIVATIONS[torso.activation], float(bounds[0]), float(bounds[1]))
    if code <= 0:
        raise NotImplementedError(lib.tonic_last_error().decode())
    return code


def _critic_count(model):
    """How many online critics the model packs: an ensemble's num_critics, 2 for twin critics, else 1."""
    if hasattr(model, 'num_critics'):
        return int(model.num_critics)
    return 2 if hasattr(model, 'critic_1') else 1


def _refuse_ensemble(name, model):
    """Every updater but TQC's two and REDQ's two on a model of N critics (models.ActorCriticEnsembleWithTargets):
    refused by name (its entries would walk N critic blocks by their own one or two)."""
    if hasattr(model, 'num_critics'):
        raise NotImplementedError(
            f'{name} does not serve a {type(model).__name__} of {model.num_critics} critics: an ensemble is trained '
            'by TQC\'s updaters, TruncatedQuantileQLearning and TwinCriticQuantileSoftPolicyGradient')


def _refuse_quantile_head(name, model):
    """The scalar and categorical updaters on a critic with a QuantileValueHead: refused by name (its block has
    neither a scalar critic's nor, without a support, a categorical critic's meaning)."""
    _refuse_ensemble(name, model)
    critic = model.critic_1 if hasattr(model, 'critic_1') else model.critic
    if hasattr(critic.head, 'num_quantiles'):
        raise NotImplementedError(
            f'{name} does not serve a critic with a QuantileValueHead: its quantiles are trained by '
            'TruncatedQuantileQLearning and TwinCriticQuantileSoftPolicyGradient (TQC)')


class _QUpdater(_FlatUpdater):
    """Shared plumbing of the four off-policy updaters: shapes, normaliser tensors, workspace."""

    head_family = 'deterministic'        # `policy_head_rule`: what this updater's entries compute at the policy's head

    # updaters whose stock-torch form exists (`_stock_enqueue`): the others keep raising for torsos
    # outside the fused kernels
    stock_capable = False

    # TQC's two updaters: the critics are QuantileValueHead networks (the others refuse such a head by name)
    quantile_critic = False

    # REDQ's two updaters: an ensemble of scalar (ValueHead) critics, packed and walked as TQC's layout at ONE output
    scalar_ensemble = False

    def _shapes(self, model):
        self.model = model
        self.observation_size = model.actor.torso.model[0].in_features
        critic = model.critic_1 if hasattr(model, 'critic_1') else model.critic
        self.quantiles = int(getattr(critic.head, 'num_quantiles', 0)) if self.quantile_critic else \
            int(self.scalar_ensemble)
        if not (self.quantile_critic or self.scalar_ensemble):
            _refuse_quantile_head(type(self).__name__, model)
        try:
            self.hidden = _torso_width(model.actor.torso, self.stock_capable)
            if _torso_width(critic.torso, self.stock_capable) != self.hidden:
                raise NotImplementedError('actor and critic torsos must have the same shape')
        except NotImplementedError:
            if not self.stock_capable:
                raise
            self.hidden = None           # any MLP(sizes, activation): stock torch operators
        head = model.actor.head
        # the torso's own code is the critic's; `hidden`, what every entry is given (each runs the actor), also carries
        # the bounds of a Gaussian head's scale — a critic ignores them
        self.torso_code, self.scale_bounds = self.hidden, None
        if self.hidden is not None:
            self.scale_bounds = policy_head_rule(head, self.head_family)
            self.hidden = _actor_code(model.actor.torso, self.scale_bounds, self.stock_capable)
        self.sac = hasattr(head, 'scale_layer')
        layer = head.loc_layer if self.sac else head.action_layer
        self.action_size = layer[0].out_features
        self.normalizer = model.observation_normalizer
        # the Return normaliser of the critics' value heads (critics.py:17-19; one module shared by the online and
        # target critics): the *_ranged entries squash with its _low / _high, read on the device
        self.return_normalizer = getattr(model, 'return_normalizer', None) or None
        device = model.flat_online.device
        self.atoms = getattr(critic.head, 'num_atoms', 0)          # > 0: distributional critic (D4PG)
        if self.normalizer is None:
            self._unit = (torch.zeros(self.observation_size, device=device),
                          torch.ones(self.observation_size, device=device))
        if self.hidden is None:
            return
        # the C side walks the flat blocks by its own offsets: both must agree on the layout
        heads = 2 if self.sac else 1
        lib = _lib.load()
        want_actor = lib.tonic_mlp_actor_param_count(
            self.observation_size, self.hidden, self.action_size, heads)
        if self.atoms:
            if not 2 <= self.atoms <= 64:
                raise NotImplementedError('the distributional kernels serve 2 .. 64 atoms')
            want_critic = lib.tonic_mlp_actor_param_count(
                self.observation_size + self.action_size, self.hidden, self.atoms, 1)
            self.values = critic.head.values.to(device=device, dtype=torch.float32).contiguous()
            # the critic step takes returns and projection from the TARGET critic's distribution
            # (critics.py:104-109); its support is the online one unless somebody changed one head
            # after the model was built (the targets are copies made at construction)
            target = getattr(model, 'target_critic', critic)
            if getattr(target.head, 'num_atoms', self.atoms) != self.atoms:
                raise NotImplementedError('online and target critic with different numbers of atoms')
            self.target_values = target.head.values.to(device=device,
                                                       dtype=torch.float32).contiguous()
        elif self.quantiles:
            want_critic = lib.tonic_mlp_actor_param_count(
                self.observation_size + self.action_size, self.hidden, self.quantiles, 1)
        else:
            want_critic = lib.tonic_q_critic_param_count(
                self.observation_size, self.action_size, self.hidden)
        n_critics = _critic_count(model)
        if (model.flat_actor.count, model.flat_critics.count) != (want_actor,
                                                                   n_critics * want_critic):
            raise NotImplementedError(
                f'network shapes outside the packed off-policy layout: actor '
                f'{model.flat_actor.count} vs {want_actor}, critics {model.flat_critics.count} '
                f'vs {n_critics} x {want_critic}')

    def norm_tensors(self):
        if self.normalizer is None:
            return self._unit
        return self.normalizer._mean.data, self.normalizer._std.data

    def norm_clip(self):
        return float(getattr(self.normalizer, 'clip', None) or 0.0)

    # agents.SAC(entropy_coeff_updater=EntropyCoeffTuning()): the SAC updaters read alpha = exp(log_entropy_coeff)
    # from the tuner's device tensor (the tonic_tempered_* entries) and their own `entropy_coeff` floats are unused
    entropy_coeff_updater = None

    def _entropy_coeff(self):
        """The stock-torch forms' alpha: the float, or — with a tuner — exp(log_entropy_coeff), kept a tensor."""
        if self.entropy_coeff_updater is None:
            return self.entropy_coeff
        return self.entropy_coeff_updater.log_entropy_coeff.detach().exp()

    def range_pointers(self):
        """Device pointers of the Return normaliser's (_low, _high); (None, None) without one: the plain heads."""
        if self.return_normalizer is None:
            return None, None
        return _lib.ptr(self.return_normalizer._low.data), _lib.ptr(self.return_normalizer._high.data)

    def _workspace_bytes(self, batch):
        """What this updater's entries ask of their workspace at `batch` rows (the hook of `_offpolicy_workspace`)."""
        shape = (batch, self.observation_size, self.action_size, self.hidden)
        if self.atoms:
            return self.lib.tonic_distributional_workspace_bytes(*shape, self.atoms)
        return self.lib.tonic_offpolicy_workspace_bytes(*shape)

    def _offpolicy_workspace(self, batch):
        need = self._workspace_bytes(batch)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.grad_sums.device)
        return self.workspace

    def enqueue_empty(self, info_row, n_global, targets=None):
        """This rank drew none of the global batch: contribute zero sums, take the same step."""
        self.grad_sums.zero_()
        self._step(n_global, info_row, targets=targets)

    def _info(self, fn, keys):
        self.scratch_info.zero_()
        fn(self.scratch_info)
        row = self.scratch_info.cpu()
        return {k: row[i].clone() for i, k in enumerate(keys)}


class TargetActionNoise:
    """critics.py:125-134 (parameters only: the clipping runs inside tonic_twin_q_grad)."""

    def __init__(self, scale=0.2, clip=0.5):
        self.scale, self.clip = scale, clip


def squashed_sample(distribution, eps):
    """SquashedMultivariateNormalDiag.rsample_with_log_prob (models/actors.py:11-16) with the
    standard-normal draws given: tanh(loc + scale * eps) and its summed log-probability."""
    normal = distribution._distribution
    raw = normal.mean + normal.stddev * eps
    squashed = torch.tanh(raw)
    log_probs = normal.log_prob(raw) - torch.log(1 - squashed ** 2 + 1e-6)
    return squashed, log_probs.sum(dim=-1)


class _TwinCriticQLearning(_QUpdater):
    stock_capable = True
    stats_kind = 3          # {loss, q1 mean, q2 mean}
    default_lr = 1e-3
    kind = 0
    loss_rule = _lib.CriticLoss()       # MSE (the distributional critic has no `loss`)

    @property
    def loss(self):
        """critics.py:58: the loss object as given (None: MSE); assigning one that is not served raises."""
        return self._loss

    @loss.setter
    def loss(self, loss):
        self.loss_rule = critic_loss_rule(loss)
        self._loss = loss

    def initialize(self, model):
        self._shapes(model)
        self._setup(model.flat_critics, optimizer_hyperparameters(self.optimizer, self.default_lr))
        self.variables = model.flat_critics.params
        if self.hidden is None:
            self._stock_setup(self.optimizer, self.default_lr)

    def _policy_params(self):
        raise NotImplementedError

    def _stock_enqueue(self, batch, eps, info_row, n_global):
        """critics.py:68-86 (kind 2), :156-182 (kind 0), :202-235 (kind 1) as stock torch operators;
        `eps` are the standard-normal draws the reference makes inside (target-action noise /
        the next action's rsample), in its order.  Losses are formed as SUMS over this rank's part
        of the batch divided by the global batch size, so that several ranks add up to the mean."""
        model, B = self.model, batch['observations'].shape[0]
        n = float(n_global or B)
        twin = hasattr(model, 'critic_1')
        with torch.no_grad():
            if self.kind == 1:
                actions, log_probs = squashed_sample(model.actor(batch['next_observations']), eps)
            else:
                actions = model.target_actor(batch['next_observations'])
                if self.kind == 0:
                    noise = self.target_action_noise
                    actions = actions + torch.clamp(noise.scale * eps, -noise.clip, noise.clip)
                    actions = torch.clamp(actions, -1, 1)
            if twin:
                next_values = torch.min(
                    model.target_critic_1(batch['next_observations'], actions),
                    model.target_critic_2(batch['next_observations'], actions))
            else:
                next_values = model.target_critic(batch['next_observations'], actions)
            if self.kind == 1:
                next_values = next_values - self._entropy_coeff() * log_probs
            returns = batch['rewards'] + batch['discounts'] * next_values
        critics = (model.critic_1, model.critic_2) if twin else (model.critic,)
        self._stock_regress(critics, batch, returns, n, info_row)

    def _stock_regress(self, critics, batch, returns, n, info_row):
        """`loss = self.loss(values, returns)` of every critic on (observations, actions), backward, the ranks'
        exchange, clip, step and the logged row {loss, mean q of each critic}."""
        from tonic_amd import parallel
        self.torch_optimizer.zero_grad()
        values = [critic(batch['observations'], batch['actions']) for critic in critics]
        loss = sum(critic_loss_sum(self.loss_rule, v, returns) for v in values) / n
        loss.backward()
        row = torch.stack([loss.detach()] + [v.detach().sum() / n for v in values])
        if parallel.exchanging():
            torch.distributed.all_reduce(row)
            for p in self.variables:
                torch.distributed.all_reduce(p.grad)
        if self.gradient_clip > 0:
            torch.nn.utils.clip_grad_norm_(self.variables, self.gradient_clip)
        self._stock_optimizer_step()
        info_row[:row.numel()] = row
        info_row[6] = 1.0

    def enqueue(self, batch, eps, info_row, n_global=None):
        if self.stock:
            return self._stock_enqueue(batch, eps, info_row, n_global)
        B = batch['observations'].shape[0]
        ws = self._offpolicy_workspace(B)
        mean, std = self.norm_tensors()
        noise = getattr(self, 'target_action_noise', None)
        p = _lib.ptr
        # (a model without a Return normaliser keeps the entry it had; with one: the squashed heads' entry)
        entry, value_range = 'tonic_twin_q_grad_loss', ()
        if self.return_normalizer is not None:
            entry, value_range = 'tonic_twin_q_grad_ranged', self.range_pointers()
        if self.entropy_coeff_updater is not None:       # (SAC: the coefficient is read on the device)
            entry = 'tonic_tempered_twin_q_grad'
            value_range = self.range_pointers() + (p(self.entropy_coeff_updater.log_entropy_coeff),)
        _lib.check(getattr(self.lib, entry)(
            self.kind, p(self._policy_params()), p(self.model.flat_target_critics.flat),
            p(self.flat.flat), p(mean), p(std), self.norm_clip(), p(batch['observations']),
            p(batch['actions']),
            p(batch['next_observations']), p(batch['rewards']), p(batch['discounts']), p(eps),
            p(self.grad_sums), B, self.observation_size, self.hidden, self.action_size,
            float(getattr(self, 'entropy_coeff', 0.0)), float(noise.scale if noise else 0.0),
            float(noise.clip if noise else 0.0), ctypes.addressof(self.loss_rule), *value_range, p(ws), ws.numel(),
            _lib.current_stream()), entry)
        self._step(n_global or B * self.world_size, info_row)

    def __call__(self, observations, actions, next_observations, rewards, discounts):
        """Drop-in form: draws its own noise from the torch CPU generator like the reference."""
        batch = dict(observations=observations, actions=actions,
                     next_observations=next_observations, rewards=rewards, discounts=discounts)
        eps = torch.randn(actions.shape).to(actions.device)
        out = self._info(lambda row: self.enqueue(batch, eps, row), ('loss', 'q1', 'q2'))
        return out


class DeterministicQLearning(_TwinCriticQLearning):
    """critics.py:56-86 (DDPG): ONE critic, target actor, no target noise."""
    kind, default_lr = 2, 1e-3

    def __init__(self, loss=None, optimizer=None, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.loss = loss
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip

    def _policy_params(self):
        return self.model.flat_target_actor.flat

    def __call__(self, observations, actions, next_observations, rewards, discounts):
        batch = dict(observations=observations, actions=actions,
                     next_observations=next_observations, rewards=rewards, discounts=discounts)
        out = self._info(lambda row: self.enqueue(batch, None, row), ('loss', 'q'))
        return out


class QRegression(_TwinCriticQLearning):
    """critics.py:31-53: ``model.critic(observations, actions)`` regressed on returns the caller computed
    (Monte-Carlo, n-step or lambda-returns of its own) — tonic_q_regression_grad + tonic_optimizer_step.  No policy
    pass and no target network: the shapes are the critic's alone, so an actor on another torso or with another head
    does not leave the HIP path, and a model needs no targets to take the stock route.

    A critic in the padded off-policy layout (``ActorCriticWithTargets.pack``) on a torso the kernels serve
    (`_torso_width`) runs the HIP entry; any other single-critic model — a torso outside the envelope,
    TONIC_AMD_TORSO_STOCK=1, a plain ``ActorCritic`` whose critic has an ObservationActionEncoder — runs the same
    arithmetic as stock torch operators.  ``__call__`` returns dict(loss=, q=) with `q` the batch mean, as
    `DeterministicQLearning` here does."""
    default_lr = 1e-3

    # (the constructor is the reference's, critics.py:33, argument for argument: a scheduler is the attribute
    #  `lr_scheduler`, assigned before `initialize`, which reads it like every other updater's)
    lr_scheduler = None

    def __init__(self, loss=None, optimizer=None, gradient_clip=0):
        self.loss = loss
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip

    def _shapes(self, model):
        from tonic_amd.torch import models
        self.model = model
        _refuse_ensemble('QRegression', model)
        if hasattr(model, 'critic_1'):
            raise NotImplementedError('QRegression regresses model.critic (critics.py:40,45): a model with critic_1 / '
                                      'critic_2 is not served, twin regression is no updater of the reference')
        critic = model.critic
        _refuse_quantile_head('QRegression', model)
        if isinstance(critic.head, models.DistributionalValueHead) or getattr(critic.head, 'num_atoms', 0):
            raise NotImplementedError('QRegression on a DistributionalValueHead is not served: the loss of '
                                      'critics.py:46 cannot take a distribution for its values')
        self.observation_size = model.actor.torso.model[0].in_features
        self.action_size = critic.torso.model[0].in_features - self.observation_size
        self.normalizer = model.observation_normalizer
        self.return_normalizer = getattr(model, 'return_normalizer', None) or None
        self.atoms, self.scale_bounds = 0, None
        # the critic's own flat block: [critic] behind the actor in the padded off-policy layout, or the unpadded
        # block of ActorCritic.pack, which only the stock route reads
        flat = getattr(model, 'flat_critics', None)
        self.hidden = None
        if flat is not None and type(critic.encoder) is models.ObservationActionEncoder and self.action_size > 0:
            try:
                self.hidden = _torso_width(critic.torso, True)
            except NotImplementedError:
                pass                         # any MLP(sizes, activation): stock torch operators
            if self.hidden is not None and flat.count != _lib.load().tonic_q_critic_param_count(
                    self.observation_size, self.action_size, self.hidden):
                self.hidden = None           # (not the packed layout the entry walks)
        if flat is None:
            flat = getattr(model, 'flat_critic', None)
        if flat is None:
            raise NotImplementedError('QRegression needs a packed model (model.pack(device)): the critic\'s '
                                      'parameters are stepped in their flat block')
        self.torso_code = self.hidden
        device = flat.flat.device
        if self.normalizer is None:
            self._unit = (torch.zeros(self.observation_size, device=device),
                          torch.ones(self.observation_size, device=device))
        return flat

    def initialize(self, model):
        flat = self._shapes(model)
        self._setup(flat, optimizer_hyperparameters(self.optimizer, self.default_lr))
        self.variables = flat.params
        if self.hidden is None:
            self._stock_setup(self.optimizer, self.default_lr)

    def _workspace_bytes(self, batch):
        return self.lib.tonic_q_regression_workspace_bytes(batch, self.observation_size, self.action_size, self.hidden)

    def _stock_enqueue(self, batch, info_row, n_global):
        """critics.py:43-53 as stock torch operators; the loss is the SUM over this rank's part of the batch divided
        by the global batch size, so that several ranks add up to the mean (`_stock_regress`)."""
        n = float(n_global or batch['observations'].shape[0])
        self._stock_regress((self.model.critic,), batch, batch['returns'], n, info_row)

    def enqueue(self, batch, info_row, n_global=None):
        """`batch`: observations [B, O], actions [B, A], returns [B] on the device.  Asynchronous; safe under a
        captured graph (the Return normaliser's range is read on the device)."""
        if self.stock:
            return self._stock_enqueue(batch, info_row, n_global)
        B = batch['observations'].shape[0]
        ws = self._offpolicy_workspace(B)
        mean, std = self.norm_tensors()
        p = _lib.ptr
        _lib.check(self.lib.tonic_q_regression_grad(
            p(self.flat.flat), p(mean), p(std), self.norm_clip(), p(batch['observations']), p(batch['actions']),
            p(batch['returns']), p(self.grad_sums), B, self.observation_size, self.hidden, self.action_size,
            ctypes.addressof(self.loss_rule), *self.range_pointers(), p(ws), ws.numel(), _lib.current_stream()),
            'tonic_q_regression_grad')
        self._step(n_global or B * self.world_size, info_row)

    def __call__(self, observations, actions, returns):
        batch = dict(observations=observations, actions=actions, returns=returns)
        return self._info(lambda row: self.enqueue(batch, row), ('loss', 'q'))


class TwinCriticDeterministicQLearning(_TwinCriticQLearning):
    """critics.py:137-182 (TD3): target actor + clipped target-action noise."""
    kind, default_lr = 0, 1e-3

    def __init__(self, loss=None, optimizer=None, target_action_noise=None, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.loss = loss
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip
        self.target_action_noise = target_action_noise or TargetActionNoise(scale=0.2, clip=0.5)

    def _policy_params(self):
        return self.model.flat_target_actor.flat


class TwinCriticSoftQLearning(_TwinCriticQLearning):
    """critics.py:185-235 (SAC): online-actor sample and entropy bonus in the target."""
    kind, default_lr = 1, 3e-4
    head_family = 'sac'

    def __init__(self, loss=None, optimizer=None, entropy_coeff=0.2, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.loss = loss
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip
        self.entropy_coeff = entropy_coeff

    def _policy_params(self):
        return self.model.flat_actor.flat


class _DistributionalQLearning(_TwinCriticQLearning):
    """The categorical critic step of D4PG and TD4: one `enqueue` for tonic_distributional_q_grad, its twin and their
    weighted forms.  A subclass names its two entries and, for the twin entry, carries a `target_action_noise`."""
    stock_capable = False
    entries = None          # (the plain entry, its weighted form)

    def _policy_params(self):
        return self.model.flat_target_actor.flat

    def _support(self):
        """The support the target distribution is projected onto."""
        raise NotImplementedError

    def enqueue(self, batch, eps, info_row, n_global=None, weights=None, sample_losses=None):
        """eps: the [B, A] standard-normal draw of the target-action noise (the twin entry; D4PG has none).
        weights / sample_losses: float32 [B] device tensors of a prioritized batch — the rows' importance weights in,
        their unweighted losses (TD4: loss_1 + loss_2) out, through the weighted entry; without them the plain one."""
        B = batch['observations'].shape[0]
        ws = self._offpolicy_workspace(B)
        mean, std = self.norm_tensors()
        noise = getattr(self, 'target_action_noise', None)
        p = _lib.ptr
        weighted = weights is not None or sample_losses is not None
        entry = self.entries[weighted]
        # the arguments every entry takes, in the prototypes' order; the twin entry's eps and noise floats and the
        # weighted entry's pair go where the prototypes have them
        networks = (p(self._policy_params()), p(self.model.flat_target_critics.flat), p(self.flat.flat), p(mean),
                    p(std), self.norm_clip())
        rows = (p(batch['observations']), p(batch['actions']), p(batch['next_observations']), p(batch['rewards']),
                p(batch['discounts']))
        sums = (p(self._support()), p(self.grad_sums), B, self.observation_size, self.hidden, self.action_size,
                self.atoms)
        workspace = (p(ws), ws.numel(), _lib.current_stream())
        draw = (p(eps),) if noise is not None else ()
        clipping = (float(noise.scale), float(noise.clip)) if noise is not None else ()
        priorities = (p(weights), p(sample_losses)) if weighted else ()
        _lib.check(getattr(self.lib, entry)(*networks, *rows, *draw, *sums, *clipping, *priorities, *workspace), entry)
        self._step(n_global or B * self.world_size, info_row)


class DistributionalDeterministicQLearning(_DistributionalQLearning):
    """critics.py:89-122 (D4PG): cross-entropy of the online critic's categorical distribution
    against the projected target distribution (tonic_distributional_q_grad)."""
    stats_kind = 4          # {loss}
    entries = ('tonic_distributional_q_grad', 'tonic_weighted_distributional_q_grad')

    def __init__(self, optimizer=None, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip

    def initialize(self, model):
        super().initialize(model)
        if not self.atoms:
            raise NotImplementedError('DistributionalDeterministicQLearning needs a critic with a '
                                      'DistributionalValueHead')

    def _support(self):
        return self.target_values          # (the TARGET head's: `_shapes`)

    def __call__(self, observations, actions, next_observations, rewards, discounts):
        batch = dict(observations=observations, actions=actions,
                     next_observations=next_observations, rewards=rewards, discounts=discounts)
        return self._info(lambda row: self.enqueue(batch, None, row), ('loss',))


class TwinCriticDistributionalDeterministicQLearning(_DistributionalQLearning):
    """TD4's critic step (the library's tensorflow/updaters/critics.py:279-336, which has no torch form): TD3's
    clipped target-action noise and twin critics on D4PG's categorical critic.  Per row, the target distribution is
    that of the target critic with the smaller mean (the first on a tie), projected onto the support at
    r + discount * z; both online critics take the cross-entropy against it (tonic_twin_distributional_q_grad).
    Logs the row of TD3 and SAC: loss, and the online critics' mean values q1, q2."""
    stats_kind = 3          # {loss, q1 mean, q2 mean}
    entries = ('tonic_twin_distributional_q_grad', 'tonic_weighted_twin_distributional_q_grad')

    def __init__(self, optimizer=None, target_action_noise=None, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip
        self.target_action_noise = target_action_noise or TargetActionNoise(scale=0.2, clip=0.5)

    def initialize(self, model):
        name = type(self).__name__
        if not hasattr(model, 'critic_2'):
            raise NotImplementedError(f'{name} needs a model with twin critics (ActorTwinCriticWithTargets)')
        _refuse_quantile_head(name, model)
        critics = (model.critic_1, model.critic_2, model.target_critic_1, model.target_critic_2)
        if not all(getattr(critic.head, 'num_atoms', 0) for critic in critics):
            raise NotImplementedError(f'{name} needs critics with a DistributionalValueHead')
        support = critics[0].head.values
        for critic in critics[1:]:
            # one support for the projection, the target means and the logged values (the targets are copies made
            # at construction: unequal only when somebody changed one head afterwards)
            if critic.head.values.shape != support.shape or not torch.equal(critic.head.values.cpu(), support.cpu()):
                raise NotImplementedError(f'{name} needs the same support in all four critics\' heads')
        super().initialize(model)

    def _support(self):
        return self.values                 # (the one support `initialize` checked all four heads to share)

    def _workspace_bytes(self, batch):
        return self.lib.tonic_twin_distributional_workspace_bytes(
            batch, self.observation_size, self.action_size, self.hidden, self.atoms)


QUANTILES_MAX = 32         # csrc/offpolicy.hip kMaxQuantiles: the two critics' pooled target values fill one wave
POOLED_MAX = 256           # csrc/offpolicy.hip kMaxPooled: an ensemble's pooled target values, four per lane


def _quantile_model(name, model):
    """What TQC's two updaters ask of the model, refused by name: twin critics or an ensemble of N, a
    QuantileValueHead of one size in all 2 N critics, 1 .. 32 quantiles, N M <= 256, no Return normaliser.  Returns
    the number of quantiles."""
    from tonic_amd.torch import models
    if not hasattr(model, 'critic_2'):
        raise NotImplementedError(f'{name} needs a model with twin critics (ActorTwinCriticWithTargets) or an '
                                  'ensemble of them (ActorCriticEnsembleWithTargets)')
    ensemble = hasattr(model, 'num_critics')
    N = _critic_count(model)
    critics = [getattr(model, f'{prefix}{z}') for prefix in ('critic_', 'target_critic_') for z in range(1, N + 1)]
    if not all(isinstance(critic.head, models.QuantileValueHead) for critic in critics):
        raise NotImplementedError(f'{name} needs critics with a QuantileValueHead')
    counts = [int(critic.head.num_quantiles) for critic in critics]
    if len(set(counts)) != 1:
        heads = f'all {2 * N}' if ensemble else 'all four'
        raise NotImplementedError(f'{name} needs the same num_quantiles in {heads} critics\' heads, got {counts}')
    if not 1 <= counts[0] <= QUANTILES_MAX:
        raise NotImplementedError(f'{name}: the quantile kernels serve num_quantiles = 1 .. {QUANTILES_MAX}, got '
                                  f'{counts[0]}')
    if ensemble and N * counts[0] > POOLED_MAX:
        raise NotImplementedError(f'{name}: the ensemble kernels pool num_critics x num_quantiles <= {POOLED_MAX} '
                                  f'values, got {N} x {counts[0]} = {N * counts[0]}')
    if getattr(model, 'return_normalizer', None):
        raise NotImplementedError(f'{name} does not serve a Return normaliser (return_normalizer): the quantile '
                                  'critics have no squashed head')
    return counts[0]


def _quantile_entry(model, step):
    """TQC's entry for `step` ('q_grad' / 'actor_grad') and what it takes behind M: a twin model keeps the twin
    entries, an ensemble (models.ActorCriticEnsembleWithTargets) takes the ensemble's with N = num_critics."""
    if hasattr(model, 'num_critics'):
        return f'tonic_ensemble_quantile_{step}', (int(model.num_critics),)
    return f'tonic_truncated_quantile_{step}', ()


def _quantile_workspace_bytes(updater, batch):
    return updater.lib.tonic_ensemble_quantile_workspace_bytes(    # (one layout: the twin model's is that of N = 2)
        batch, updater.observation_size, updater.action_size, updater.hidden, updater.quantiles,
        _critic_count(updater.model))


class TruncatedQuantileQLearning(_TwinCriticQLearning):
    """TQC's critic step (Kuznetsov et al. 2020; the reference has none): SAC's — the ONLINE actor's sample at s' and
    its entropy bonus in the target — on two critics of M quantiles each.  Per row the two target critics' 2 M values
    are pooled and sorted and the `top_quantiles_to_drop_per_net` largest per critic dropped, K = 2 (M - d) kept:
    y_j = r + discount (Z_j - alpha logp'); each online critic takes the quantile Huber loss (kappa = 1) of its M
    quantiles at tau_i = (2 i + 1) / (2 M) against the K targets, loss_1 + loss_2 (tonic_truncated_quantile_q_grad).
    Logs the row of SAC: loss, and the online critics' mean quantiles q1, q2.
    On an ensemble of N critics (models.ActorCriticEnsembleWithTargets): the same with 2 -> N, N M <= 256
    (tonic_ensemble_quantile_q_grad); the row is then loss and q, the mean over the critics."""
    kind, default_lr = 1, 3e-4
    head_family = 'sac'
    stock_capable = False
    quantile_critic = True

    def __init__(self, optimizer=None, entropy_coeff=0.2, top_quantiles_to_drop_per_net=2, gradient_clip=0,
                 lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.optimizer = optimizer
        self.entropy_coeff = entropy_coeff
        self.top_quantiles_to_drop_per_net = top_quantiles_to_drop_per_net
        self.gradient_clip = gradient_clip

    def initialize(self, model):
        name = type(self).__name__
        quantiles = _quantile_model(name, model)
        drop = self.top_quantiles_to_drop_per_net
        if int(drop) != drop or not 0 <= drop < quantiles:
            raise NotImplementedError(f'{name}: top_quantiles_to_drop_per_net = 0 .. num_quantiles - 1 = '
                                      f'{quantiles - 1}, got {drop!r}')
        super().initialize(model)

    def _policy_params(self):
        return self.model.flat_actor.flat

    def _workspace_bytes(self, batch):
        return _quantile_workspace_bytes(self, batch)

    def enqueue(self, batch, eps, info_row, n_global=None):
        """eps: the [B, A] standard-normal draw of the next action's rsample."""
        B = batch['observations'].shape[0]
        ws = self._offpolicy_workspace(B)
        mean, std = self.norm_tensors()
        p = _lib.ptr
        tuner = self.entropy_coeff_updater         # (the coefficient is then read on the device)
        entry, ensemble = _quantile_entry(self.model, 'q_grad')
        _lib.check(getattr(self.lib, entry)(
            p(self._policy_params()), p(self.model.flat_target_critics.flat), p(self.flat.flat), p(mean), p(std),
            self.norm_clip(), p(batch['observations']), p(batch['actions']), p(batch['next_observations']),
            p(batch['rewards']), p(batch['discounts']), p(eps), p(self.grad_sums), B, self.observation_size,
            self.hidden, self.action_size, self.quantiles, *ensemble, int(self.top_quantiles_to_drop_per_net),
            float(self.entropy_coeff), p(tuner.log_entropy_coeff) if tuner is not None else None, p(ws), ws.numel(),
            _lib.current_stream()), entry)
        self._step(n_global or B * self.world_size, info_row)

    def __call__(self, observations, actions, next_observations, rewards, discounts):
        out = super().__call__(observations, actions, next_observations, rewards, discounts)
        if hasattr(self.model, 'num_critics'):       # (an ensemble's row: loss and the mean q over its critics)
            out = {'loss': out['loss'], 'q': out['q1']}
        return out


def _ensemble_model(name, model):
    """What REDQ's two updaters ask of the model, refused by name: an ensemble (models.ActorCriticEnsembleWithTargets)
    whose 2 N critics all have a plain ValueHead, no Return normaliser, and torsos the kernels run."""
    from tonic_amd.torch import models
    if not isinstance(model, models.ActorCriticEnsembleWithTargets):
        raise NotImplementedError(f'{name} needs an ensemble of critics (models.ActorCriticEnsembleWithTargets), got a '
                                  f'{type(model).__name__}')
    heads = [type(critic.head) for critic in model.critics() + model.critics(target=True)]
    if any(head is not models.ValueHead for head in heads):       # (a subclass may compute anything in its forward)
        raise NotImplementedError(f'{name} needs critics with a ValueHead (one value each), all {len(heads)} of them, '
                                  f'got {[head.__name__ for head in heads]}')
    if getattr(model, 'return_normalizer', None):
        raise NotImplementedError(f'{name} does not serve a Return normaliser (return_normalizer='
                                  f'{type(model.return_normalizer).__name__}): the ensemble kernels have no squashed head')
    for role, network in (('actor', model.actor), ('critic', model.critic_1)):
        try:
            _torso_width(network.torso)
        except NotImplementedError as error:
            raise NotImplementedError(f'{name}: the {role}\'s torso: {error}') from None


def subset_mask(critics):
    """The device word of a subset: bit z set for every critic index z (0-based) in `critics`."""
    mask = 0
    for z in critics:
        mask |= 1 << int(z)
    return mask


def draw_subset_masks(generator, iterations, num_critics, subset_size):
    """REDQ's subset stream: int32 [iterations], one mask per learner iteration with `subset_size` distinct critics of
    `num_critics`, uniform over the subsets, each iteration one draw of `generator` (a numpy RandomState) — the stream
    is the same however the iterations are split into calls.  subset_size == num_critics: the minimum over all
    critics, which draws nothing."""
    if subset_size == num_critics:
        return np.full(iterations, (1 << num_critics) - 1, np.int32)
    return np.array([subset_mask(generator.choice(num_critics, size=subset_size, replace=False))
                     for _ in range(iterations)], np.int32).reshape(iterations)


class EnsembleSoftQLearning(_TwinCriticQLearning):
    """REDQ's critic step (Chen et al. 2021, randomized ensembled double Q-learning; the reference has none): SAC's —
    the ONLINE actor's sample at s' and its entropy bonus in the target — on an ensemble of N scalar critics
    (models.ActorCriticEnsembleWithTargets with ValueHead critics).  Per update a subset S of `subset_size` target
    critics is named by one int32 on the device (bit z: critic z + 1), y = r + discount (min_{z in S} Qt_z(s', a') -
    alpha logp'), and ALL N online critics regress on y with `loss` (tonic_ensemble_subset_q_grad).  The agent draws
    the subsets (`draw_subset_masks`); the kernel reads the word, so a captured update graph follows them.
    subset_size == num_critics is the minimum over all critics.  Logs the ensemble's row: loss, and q, the mean over
    the critics."""
    kind, default_lr = 1, 3e-4
    head_family = 'sac'
    stock_capable = False
    scalar_ensemble = True
    takes_subset = True          # (`QUpdate`: enqueue takes the pointer of the iteration's word)

    def __init__(self, loss=None, optimizer=None, entropy_coeff=0.2, subset_size=2, gradient_clip=0,
                 lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        try:
            self.loss = loss
        except NotImplementedError as error:
            raise NotImplementedError(f'{type(self).__name__}: {error}') from None
        self.optimizer = optimizer
        self.entropy_coeff = entropy_coeff
        self.subset_size = subset_size
        self.gradient_clip = gradient_clip

    def initialize(self, model):
        name = type(self).__name__
        _ensemble_model(name, model)
        size, N = self.subset_size, model.num_critics
        whole = isinstance(size, (int, float)) and not isinstance(size, bool) and int(size) == size
        if not whole or not 1 <= size <= N:
            raise NotImplementedError(f'{name}: subset_size is a whole number in 1 .. num_critics = {N}, got {size!r}')
        self.subset_size = int(size)
        try:
            self.loss = self._loss         # (anew: whoever assigned `_loss` directly is told here)
        except NotImplementedError as error:
            raise NotImplementedError(f'{name}: {error}') from None
        super().initialize(model)
        self._subset = torch.zeros(1, dtype=torch.int32, device=model.flat_online.device)

    def _policy_params(self):
        return self.model.flat_actor.flat

    def _workspace_bytes(self, batch):
        return self.lib.tonic_ensemble_q_workspace_bytes(batch, self.observation_size, self.action_size, self.hidden,
                                                         _critic_count(self.model))

    def enqueue(self, batch, eps, info_row, n_global=None, subset=None):
        """eps: the [B, A] standard-normal draw of the next action's rsample; subset: an int32 device tensor whose
        first element is the subset's mask (None: the word `__call__` filled)."""
        B = batch['observations'].shape[0]
        ws = self._offpolicy_workspace(B)
        mean, std = self.norm_tensors()
        p = _lib.ptr
        tuner = self.entropy_coeff_updater         # (the coefficient is then read on the device)
        entry = 'tonic_ensemble_subset_q_grad'
        _lib.check(getattr(self.lib, entry)(
            p(self._policy_params()), p(self.model.flat_target_critics.flat), p(self.flat.flat), p(mean), p(std),
            self.norm_clip(), p(batch['observations']), p(batch['actions']), p(batch['next_observations']),
            p(batch['rewards']), p(batch['discounts']), p(eps), p(self.grad_sums), B, self.observation_size,
            self.hidden, self.action_size, _critic_count(self.model), p(self._subset if subset is None else subset),
            float(self.entropy_coeff), p(tuner.log_entropy_coeff) if tuner is not None else None,
            ctypes.addressof(self.loss_rule), p(ws), ws.numel(), _lib.current_stream()), entry)
        self._step(n_global or B * self.world_size, info_row)

    def __call__(self, observations, actions, next_observations, rewards, discounts, subset=None):
        """Drop-in form: draws its own noise from the torch CPU generator and, unless `subset` (a mask) is given, its
        subset from numpy's global RandomState."""
        if subset is None:
            subset = draw_subset_masks(np.random, 1, _critic_count(self.model), self.subset_size)[0]
        self._subset.fill_(int(subset))
        out = super().__call__(observations, actions, next_observations, rewards, discounts)
        return {'loss': out['loss'], 'q': out['q1']}


class ExpectedSARSA(_TwinCriticQLearning):
    """critics.py:238-282 (MPO): one critic regressed on r + discount * the mean target value of
    `num_samples` actions drawn from the target actor (tonic_expected_sarsa_grad)."""
    default_lr = 3e-4
    stock_capable = False
    head_family = 'mpo'

    def __init__(self, num_samples=20, loss=None, optimizer=None, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        _check_num_samples('ExpectedSARSA', num_samples)
        self.loss = loss
        self.num_samples = num_samples
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip

    def initialize(self, model):
        _refuse_ensemble(type(self).__name__, model)
        critic = model.critic_1 if hasattr(model, 'critic_1') else model.critic
        if getattr(critic.head, 'num_atoms', 0):
            # (the scalar entry would walk the categorical critic's block by a scalar critic's offsets)
            raise NotImplementedError('ExpectedSARSA regresses a scalar critic: a critic with a '
                                      'DistributionalValueHead takes DistributionalExpectedSARSA')
        super().initialize(model)

    def _workspace_bytes(self, batch):
        return self.lib.tonic_mpo_workspace_bytes(batch, self.observation_size, self.action_size, self.hidden,
                                                  self.num_samples)

    def enqueue(self, batch, eps, info_row, n_global=None):
        """eps: the [num_samples * B, A] standard-normal draws of `rsample((num_samples,))`."""
        B = batch['observations'].shape[0]
        ws = self._offpolicy_workspace(B)
        mean, std = self.norm_tensors()
        p = _lib.ptr
        _lib.check(self.lib.tonic_expected_sarsa_grad_loss(
            p(self.model.flat_target_actor.flat), p(self.model.flat_target_critics.flat),
            p(self.flat.flat), p(mean), p(std), self.norm_clip(), p(batch['observations']),
            p(batch['actions']), p(batch['next_observations']), p(batch['rewards']),
            p(batch['discounts']), p(eps), p(self.grad_sums), B, self.observation_size, self.hidden,
            self.action_size, self.num_samples, ctypes.addressof(self.loss_rule), p(ws), ws.numel(),
            _lib.current_stream()), 'tonic_expected_sarsa_grad_loss')
        self._step(n_global or B, info_row)

    def __call__(self, observations, actions, next_observations, rewards, discounts):
        batch = dict(observations=observations, actions=actions,
                     next_observations=next_observations, rewards=rewards, discounts=discounts)
        eps = torch.randn(self.num_samples * observations.shape[0], self.action_size).to(
            observations.device)
        return self._info(lambda row: self.enqueue(batch, eps, row), ('loss', 'q'))


class DistributionalExpectedSARSA(_TwinCriticQLearning):
    """DMPO's critic step, which no reference line states: ExpectedSARSA on D4PG's categorical critic.  Per row the
    target is the MIXTURE of the target critic's distributions at `num_samples` actions drawn from the target actor,
    projected onto the support at r + discount * z (CategoricalWithSupport.project is linear in the distribution, so
    the mixture is projected once); the online critic takes the cross-entropy against it
    (tonic_distributional_expected_sarsa_grad).  Logs ExpectedSARSA's row: loss, and the online critic's mean value q."""
    default_lr = 3e-4
    stock_capable = False
    head_family = 'mpo'
    stats_kind = 3          # {loss, q mean}

    def __init__(self, num_samples=20, optimizer=None, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        _check_num_samples('DistributionalExpectedSARSA', num_samples)
        self.num_samples = num_samples
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip

    def initialize(self, model):
        name = type(self).__name__
        _refuse_ensemble(name, model)
        if hasattr(model, 'critic_1'):
            raise NotImplementedError(f'{name} serves one critic with its target (ActorCriticWithTargets), not twin '
                                      'critics')
        _refuse_quantile_head(name, model)
        if not getattr(model.critic.head, 'num_atoms', 0):
            raise NotImplementedError(f'{name} needs a critic with a DistributionalValueHead')
        online, target = model.critic.head.values, model.target_critic.head.values
        if online.shape != target.shape or not torch.equal(online.cpu(), target.cpu()):
            # one support for the projection and the logged values (the target is a copy made at construction:
            # unequal only when somebody changed one head afterwards)
            raise NotImplementedError(f'{name} needs the same support in the online and the target critic\'s heads')
        super().initialize(model)

    def _workspace_bytes(self, batch):
        return self.lib.tonic_distributional_mpo_workspace_bytes(
            batch, self.observation_size, self.action_size, self.hidden, self.num_samples, self.atoms)

    def enqueue(self, batch, eps, info_row, n_global=None):
        """eps: the [num_samples * B, A] standard-normal draws of the target actor's `rsample((num_samples,))`."""
        B = batch['observations'].shape[0]
        ws = self._offpolicy_workspace(B)
        mean, std = self.norm_tensors()
        p = _lib.ptr
        _lib.check(self.lib.tonic_distributional_expected_sarsa_grad(
            p(self.model.flat_target_actor.flat), p(self.model.flat_target_critics.flat),
            p(self.flat.flat), p(mean), p(std), self.norm_clip(), p(batch['observations']),
            p(batch['actions']), p(batch['next_observations']), p(batch['rewards']),
            p(batch['discounts']), p(eps), p(self.target_values), p(self.grad_sums), B, self.observation_size,
            self.hidden, self.action_size, self.num_samples, self.atoms, p(ws), ws.numel(),
            _lib.current_stream()), 'tonic_distributional_expected_sarsa_grad')
        self._step(n_global or B, info_row)

    def __call__(self, observations, actions, next_observations, rewards, discounts):
        batch = dict(observations=observations, actions=actions,
                     next_observations=next_observations, rewards=rewards, discounts=discounts)
        eps = torch.randn(self.num_samples * observations.shape[0], self.action_size).to(
            observations.device)
        return self._info(lambda row: self.enqueue(batch, eps, row), ('loss', 'q'))


class _ActorQGradient(_QUpdater):
    stock_capable = True
    stats_kind = 4          # {loss}
    default_lr = 1e-3
    kind = 0

    def initialize(self, model):
        self._shapes(model)
        self._setup(model.flat_actor, optimizer_hyperparameters(self.optimizer, self.default_lr))
        self.variables = model.flat_actor.params
        if self.hidden is None:
            self._stock_setup(self.optimizer, self.default_lr)

    def _stock_enqueue(self, observations, eps, info_row, n_global, targets):
        """actors.py:170-189 (kind 0: -mean q of `model.critic`) / :238-267 (kind 1: mean of
        alpha log-prob - min q) as stock torch operators; only the actor's variables receive
        gradients (the reference freezes the critics around its backward)."""
        from tonic_amd import parallel
        model, B = self.model, observations.shape[0]
        n = float(n_global or B)
        if self.kind == 1:
            actions, log_probs = squashed_sample(model.actor(observations), eps)
            values = torch.min(model.critic_1(observations, actions),
                               model.critic_2(observations, actions))
            loss = (self._entropy_coeff() * log_probs - values).sum() / n
            if self.entropy_coeff_updater is not None:      # the coefficient's sums from the same log-probabilities
                self.entropy_coeff_updater.stock_sums(log_probs.detach())
        else:
            critic = model.critic if hasattr(model, 'critic') else model.critic_1
            loss = -critic(observations, model.actor(observations)).sum() / n
        grads = torch.autograd.grad(loss, self.variables)
        row = loss.detach().reshape(1)
        for p, grad in zip(self.variables, grads):
            p.grad = grad
        if parallel.exchanging():
            torch.distributed.all_reduce(row)
            for p in self.variables:
                torch.distributed.all_reduce(p.grad)
        if self.gradient_clip > 0:
            torch.nn.utils.clip_grad_norm_(self.variables, self.gradient_clip)
        self._stock_optimizer_step()
        info_row[0] = row[0]
        info_row[6] = 1.0
        if targets is not None:                         # update_targets right after (ddpg.py:112)
            model.update_targets()

    def enqueue(self, observations, eps, info_row, n_global=None, targets=None):
        if self.stock:
            return self._stock_enqueue(observations, eps, info_row, n_global, targets)
        B = observations.shape[0]
        ws = self._offpolicy_workspace(B)
        mean, std = self.norm_tensors()
        p = _lib.ptr
        entry, value_range = 'tonic_actor_q_grad', ()
        if self.return_normalizer is not None:
            entry, value_range = 'tonic_actor_q_grad_ranged', self.range_pointers()
        tuner = self.entropy_coeff_updater
        if tuner is not None:                            # (SAC: the coefficient is read, its sums written, on the device)
            entry = 'tonic_tempered_actor_q_grad'
            value_range = self.range_pointers() + (p(tuner.log_entropy_coeff), p(tuner.grad_sums),
                                                   float(tuner.target_entropy))
        _lib.check(getattr(self.lib, entry)(
            self.kind, p(self.flat.flat), p(self.model.flat_critics.flat), p(mean), p(std),
            self.norm_clip(), p(observations), p(eps), p(self.grad_sums), B, self.observation_size, self.hidden,
            self.action_size, float(getattr(self, 'entropy_coeff', 0.0)), *value_range, p(ws), ws.numel(),
            _lib.current_stream()), entry)
        self._step(n_global or B * self.world_size, info_row, targets=targets)

    def __call__(self, observations):
        eps = None
        if self.kind == 1:
            eps = torch.randn(observations.shape[0], self.action_size).to(observations.device)
        return self._info(lambda row: self.enqueue(observations, eps, row), ('loss',))


class DeterministicPolicyGradient(_ActorQGradient):
    """actors.py:159-189 on `model.critic` (= critic_1 for TD3, td3.py:36)."""
    kind, default_lr = 0, 1e-3

    def __init__(self, optimizer=None, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip


class DistributionalDeterministicPolicyGradient(_ActorQGradient):
    """actors.py:192-224 (D4PG): ascend the mean of the critic's value distribution
    (tonic_distributional_actor_grad)."""
    stock_capable = False

    def __init__(self, optimizer=None, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip

    def initialize(self, model):
        super().initialize(model)
        if not self.atoms:
            raise NotImplementedError('DistributionalDeterministicPolicyGradient needs a critic '
                                      'with a DistributionalValueHead')

    def enqueue(self, observations, eps, info_row, n_global=None, targets=None):
        B = observations.shape[0]
        ws = self._offpolicy_workspace(B)
        mean, std = self.norm_tensors()
        p = _lib.ptr
        _lib.check(self.lib.tonic_distributional_actor_grad(
            p(self.flat.flat), p(self.model.flat_critics.flat), p(mean), p(std), self.norm_clip(),
            p(observations), p(self.values), p(self.grad_sums), B, self.observation_size,
            self.hidden, self.action_size, self.atoms, p(ws), ws.numel(), _lib.current_stream()),
            'tonic_distributional_actor_grad')
        self._step(n_global or B * self.world_size, info_row, targets=targets)


MPO_MAX_SAMPLES = 256      # csrc/offpolicy.hip kMpoMaxSamples: four register slots per lane in the E-step


def _check_num_samples(name, num_samples):
    if not 1 <= int(num_samples) <= MPO_MAX_SAMPLES:
        raise NotImplementedError(
            f'{name}(num_samples={num_samples}): the MPO kernels hold 1 <= num_samples <= {MPO_MAX_SAMPLES} '
            'samples per state')


MPO_INFO = ('policy_mean_loss', 'policy_std_loss', 'kl_mean_loss', 'kl_std_loss', 'alpha_mean_loss',
            'alpha_std_loss', 'temperature_loss', 'temperature')


class MaximumAPosterioriPolicyOptimization(_ActorQGradient):
    """actors.py:270-464 (tonic_mpo_actor_grad_joint): the actor step and the step of the dual variables
    {log_temperature, log_alpha_mean[K], log_alpha_std[K], log_penalty_temperature} — K = A with per-dimension
    KL constraints, K = 1 with `per_dim_constraining=False` (one alpha pair on the KLs summed over the action
    dimensions) — one flat device vector with its own Adam state (actors.py:289-316; like the reference, the
    dual optimizer is Adam(lr=1e-2) unless `actor_optimizer` is given).  On a critic with a DistributionalValueHead
    (DMPO) the E-step's values are the means of the target critic's distributions
    (tonic_distributional_mpo_actor_grad); everything else is the same step."""
    default_lr = 3e-4
    stock_capable = False
    head_family = 'mpo'

    def __init__(self, num_samples=20, epsilon=1e-1, epsilon_penalty=1e-3, epsilon_mean=1e-3,
                 epsilon_std=1e-6, initial_log_temperature=1., initial_log_alpha_mean=1.,
                 initial_log_alpha_std=10., min_log_dual=-18., per_dim_constraining=True,
                 action_penalization=True, actor_optimizer=None, dual_optimizer=None,
                 gradient_clip=0, actor_lr_scheduler=None, dual_lr_scheduler=None):
        _check_num_samples('MaximumAPosterioriPolicyOptimization', num_samples)
        self.num_samples = num_samples
        self.per_dim_constraining = per_dim_constraining
        self.epsilon, self.epsilon_penalty = epsilon, epsilon_penalty
        self.epsilon_mean, self.epsilon_std = epsilon_mean, epsilon_std
        self.initial_log_temperature = initial_log_temperature
        self.initial_log_alpha_mean = initial_log_alpha_mean
        self.initial_log_alpha_std = initial_log_alpha_std
        self.min_log_dual = min_log_dual
        self.action_penalization = action_penalization
        self.optimizer = actor_optimizer
        self.dual_hyper = optimizer_hyperparameters(actor_optimizer, 1e-2)      # actors.py:291-292
        self.gradient_clip = gradient_clip
        self.lr_scheduler, self.dual_lr_scheduler = actor_lr_scheduler, dual_lr_scheduler
        self.dual_schedule = lr_schedule_rule(dual_lr_scheduler, actor_optimizer, 1e-2)   # (the duals' own count)

    def initialize(self, model, action_space=None):
        super().initialize(model)
        A, device = self.action_size, self.grad_sums.device
        K = self.constraints = A if self.per_dim_constraining else 1        # actors.py:300-311
        duals = [self.initial_log_temperature] + [self.initial_log_alpha_mean] * K + \
            [self.initial_log_alpha_std] * K + [self.initial_log_temperature]
        self.duals = torch.tensor(duals, dtype=torch.float32, device=device)
        self.dual_grads = torch.zeros(2 * K + 2 + INFO_WIDTH, dtype=torch.float32, device=device)
        self.dual_optim = _OptimizerState(self.lib, self.dual_hyper, 2 * K + 2, device, self.dual_schedule)
        self.dual_slots, self.dual_state = self.dual_optim.slots, self.dual_optim.state
        self.dual_exp_avg, self.dual_exp_avg_sq = self.dual_optim.exp_avg, self.dual_optim.exp_avg_sq
        self.mpo_stats = torch.zeros(9 + 2 * K, dtype=torch.float32, device=device)
        self.dual_info = torch.zeros(INFO_WIDTH, dtype=torch.float32, device=device)
        self.column_sums = torch.zeros(6 + 2 * A, dtype=torch.float64, device=device)
        self.dual_clip_workspace = torch.zeros(
            self.lib.tonic_clip_workspace_bytes(2 * K + 2), dtype=torch.uint8, device=device)

    def _workspace_bytes(self, batch):
        shape = (batch, self.observation_size, self.action_size, self.hidden, self.num_samples)
        if self.atoms:
            return self.lib.tonic_distributional_mpo_workspace_bytes(*shape, self.atoms)
        return self.lib.tonic_mpo_workspace_bytes(*shape)

    def enqueue(self, observations, eps, info_row, n_global=None, targets=None, stats_row=None):
        from tonic_amd import parallel
        p = _lib.ptr
        # a categorical target critic (DMPO): the tonic_distributional_mpo_* entries, which take the TARGET head's
        # support (`_shapes`) behind eps and the number of atoms behind the samples; else the calls as they were
        whole, shard = 'tonic_mpo_actor_grad_joint', 'tonic_mpo_actor_grad_shard_joint'
        support, atoms = (), ()
        if self.atoms:
            whole, shard = 'tonic_distributional_mpo_actor_grad', 'tonic_distributional_mpo_actor_grad_shard'
            support, atoms = (p(self.target_values),), (self.atoms,)
        # (actors.py:347-356 floors the log-duals in place at the head of the call: the kernels read them
        #  through the floor and write the floored values back ahead of the duals' optimizer step)
        floor, joint = float(self.min_log_dual), int(not self.per_dim_constraining)
        stats = stats_row if stats_row is not None else self.mpo_stats
        B = 0 if observations is None else observations.shape[0]
        if parallel.exchanging():
            # this rank's part of the global batch (possibly nothing): the actor's gradient sums and
            # the column sums of the per-state terms (per-dimension KLs, whatever the constraint); the dual
            # step needs their GLOBAL means
            if B > 0:
                ws = self._offpolicy_workspace(B)
                mean, std = self.norm_tensors()
                _lib.check(getattr(self.lib, shard)(
                    p(self.flat.flat), p(self.model.flat_target_actor.flat),
                    p(self.model.flat_target_critics.flat), p(self.duals), floor, p(mean), p(std),
                    self.norm_clip(), p(observations), p(eps), *support, p(self.grad_sums),
                    p(self.column_sums), B, self.observation_size, self.hidden, self.action_size,
                    self.num_samples, *atoms, int(bool(self.action_penalization)), joint, p(ws), ws.numel(),
                    _lib.current_stream()), shard)
            else:
                self.grad_sums.zero_()
                self.column_sums.zero_()
            torch.distributed.all_reduce(self.column_sums)
            _lib.check(self.lib.tonic_mpo_dual_step_joint(
                p(self.column_sums), p(self.duals), floor, p(self.dual_grads), p(stats),
                p(self.grad_sums[self.count:]), B, n_global, self.action_size, self.num_samples,
                float(self.epsilon), float(self.epsilon_penalty), float(self.epsilon_mean),
                float(self.epsilon_std), int(bool(self.action_penalization)), joint,
                _lib.current_stream()), 'tonic_mpo_dual_step_joint')
        else:
            ws = self._offpolicy_workspace(B)
            mean, std = self.norm_tensors()
            _lib.check(getattr(self.lib, whole)(
                p(self.flat.flat), p(self.model.flat_target_actor.flat),
                p(self.model.flat_target_critics.flat), p(self.duals), floor, p(mean), p(std),
                self.norm_clip(), p(observations), p(eps), *support, p(self.grad_sums), p(self.dual_grads),
                p(stats), B, self.observation_size, self.hidden, self.action_size,
                self.num_samples, *atoms, float(self.epsilon), float(self.epsilon_penalty),
                float(self.epsilon_mean), float(self.epsilon_std),
                int(bool(self.action_penalization)), joint, p(ws), ws.numel(), _lib.current_stream()),
                whole)
        self._step(n_global or B, info_row, targets=targets)
        if self.gradient_clip > 0:
            # actors.py:441-445 clips the dual variables' gradient norm as well (the penalty
            # temperature's entry is zero without action penalisation, so it does not count)
            _lib.check(self.lib.tonic_clip_grad_norm(
                p(self.dual_grads), self.duals.numel(), 1.0, self.gradient_clip, None,
                p(self.dual_clip_workspace), self.dual_clip_workspace.numel(),
                _lib.current_stream()), 'tonic_clip_grad_norm (duals)')
        self.dual_optim.enqueue(self.duals, self.dual_grads, 1.0, self.dual_info,
                                what='tonic_optimizer_step (duals)')

    def enqueue_empty(self, info_row, n_global, targets=None, stats_row=None):
        """This rank drew none of the global batch: zero sums, the same dual and actor steps."""
        self.enqueue(None, None, info_row, n_global, targets, stats_row)

    def infos(self, stats):
        """The reference's return dict (actors.py:449-464) from one statistics row (host array)."""
        K = self.constraints
        out = {k: stats[i] for i, k in enumerate(MPO_INFO)}
        out['alpha_mean'] = stats[8:8 + K]
        out['alpha_std'] = stats[8 + K:8 + 2 * K]
        if self.action_penalization:
            out['penalty_temperature'] = stats[8 + 2 * K]
        return out

    def __call__(self, observations):
        eps = torch.randn(self.num_samples * observations.shape[0], self.action_size).to(
            observations.device)
        self.scratch_info.zero_()
        self.enqueue(observations, eps, self.scratch_info)
        return {k: torch.as_tensor(v) for k, v in self.infos(self.mpo_stats.cpu().numpy()).items()}


class TwinCriticSoftDeterministicPolicyGradient(_ActorQGradient):
    """actors.py:226-267 (SAC)."""
    kind, default_lr = 1, 3e-4
    head_family = 'sac'

    def __init__(self, optimizer=None, entropy_coeff=0.2, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip
        self.entropy_coeff = entropy_coeff


class TwinCriticQuantileSoftPolicyGradient(_ActorQGradient):
    """TQC's actor step: SAC's (actors.py:226-267) with the mean of the two online critics' 2 M quantiles in the place
    of min(q1, q2): loss = mean(alpha logp - Q) (tonic_truncated_quantile_actor_grad).  With a tuner the entry also
    writes the coefficient's block, as SAC's tempered entry does.  On an ensemble of N critics: the mean of their N M
    quantiles (tonic_ensemble_quantile_actor_grad)."""
    kind, default_lr = 1, 3e-4
    head_family = 'sac'
    stock_capable = False
    quantile_critic = True

    def __init__(self, optimizer=None, entropy_coeff=0.2, gradient_clip=0, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        self.optimizer = optimizer
        self.gradient_clip = gradient_clip
        self.entropy_coeff = entropy_coeff

    def initialize(self, model):
        _quantile_model(type(self).__name__, model)
        super().initialize(model)

    def _workspace_bytes(self, batch):
        return _quantile_workspace_bytes(self, batch)

    def enqueue(self, observations, eps, info_row, n_global=None, targets=None):
        B = observations.shape[0]
        ws = self._offpolicy_workspace(B)
        mean, std = self.norm_tensors()
        p = _lib.ptr
        tuner = self.entropy_coeff_updater
        temper = (None, None, 0.0) if tuner is None else (p(tuner.log_entropy_coeff), p(tuner.grad_sums),
                                                          float(tuner.target_entropy))
        entry, ensemble = _quantile_entry(self.model, 'actor_grad')
        _lib.check(getattr(self.lib, entry)(
            p(self.flat.flat), p(self.model.flat_critics.flat), p(mean), p(std), self.norm_clip(), p(observations),
            p(eps), p(self.grad_sums), B, self.observation_size, self.hidden, self.action_size, self.quantiles,
            *ensemble, float(self.entropy_coeff), *temper, p(ws), ws.numel(), _lib.current_stream()), entry)
        self._step(n_global or B * self.world_size, info_row, targets=targets)


class EnsembleSoftPolicyGradient(TwinCriticQuantileSoftPolicyGradient):
    """REDQ's actor step: SAC's (actors.py:226-267) with the mean of ALL N online critics in the place of
    min(q1, q2): loss = mean(alpha logp - (1 / N) sum_z Q_z).  N critics of one output each are TQC's ensemble at
    M = 1, so the step is tonic_ensemble_quantile_actor_grad at M = 1, the tuner's block included."""
    quantile_critic = False
    scalar_ensemble = True

    def initialize(self, model):
        _ensemble_model(type(self).__name__, model)
        _ActorQGradient.initialize(self, model)


class EntropyCoeffTuning(_FlatUpdater):
    """SAC's automatic temperature adjustment (Haarnoja et al. 2018b, section 5; the reference keeps its 0.2): the
    entropy coefficient alpha = exp(log_entropy_coeff) descends J = -mean(log_entropy_coeff * (log_probs +
    target_entropy)) on the log-probabilities of the actor step's own sample.  `log_entropy_coeff` is ONE float32 on
    the device; the SAC updaters' tonic_tempered_* entries read it there and tonic_tempered_actor_q_grad writes the
    gradient sum and the statistics into `grad_sums` [1 + 8], which steps through tonic_optimizer_step like every
    other block (any rule of `optimizer_hyperparameters`, the ranks' exchange included).  The host never reads the
    coefficient during training: a captured update graph follows it.

    target_entropy          None: -action_size, resolved at `initialize`
    initial_entropy_coeff   alpha before the first step (> 0, finite)
    optimizer               reference style, ``lambda params: torch.optim.X(params, ...)``; default Adam(lr=3e-4)"""

    stats_kind = 3          # {loss, mean log-prob, alpha before the step}
    default_lr = 3e-4
    INFO = ('loss', 'log_prob', 'value')

    def __init__(self, target_entropy=None, initial_entropy_coeff=1.0, optimizer=None, lr_scheduler=None):
        self.lr_scheduler = lr_scheduler
        initial = float(initial_entropy_coeff)
        if not (math.isfinite(initial) and initial > 0):
            raise ValueError(f'initial_entropy_coeff={initial_entropy_coeff!r}: the coefficient is exp(log_entropy_coeff), '
                             'a finite number above 0')
        if target_entropy is not None and not math.isfinite(float(target_entropy)):
            raise ValueError(f'target_entropy={target_entropy!r} is not finite')
        self.target_entropy = None if target_entropy is None else float(target_entropy)
        self.initial_entropy_coeff = initial
        self.optimizer = optimizer
        self.hyper = optimizer_hyperparameters(optimizer, self.default_lr)      # (the refusals, by name, right here)
        lr_schedule_rule(lr_scheduler, optimizer, self.default_lr)
        self.log_entropy_coeff = None

    def initialize(self, model, action_size=None):
        if action_size is None:
            action_size = model.actor.head.loc_layer[0].out_features
        if self.target_entropy is None:
            self.target_entropy = -float(action_size)
        device = model.flat_online.device
        self.log_entropy_coeff = torch.full((1,), math.log(self.initial_entropy_coeff), dtype=torch.float32,
                                            device=device)
        self._setup(types.SimpleNamespace(flat=self.log_entropy_coeff, count=1),
                    optimizer_hyperparameters(self.optimizer, self.default_lr))
        self.variables = [self.log_entropy_coeff]

    @property
    def entropy_coeff(self):
        """alpha as a Python float (one read-back: for logs and tests, never on the update path)."""
        return float(self.log_entropy_coeff.exp())

    def stock_sums(self, log_probs):
        """`grad_sums` as tonic_tempered_actor_q_grad writes it, from stock torch operators (the stock-torch actor
        step: the same layout, so the step and the ranks' exchange are the same)."""
        log_alpha = self.log_entropy_coeff.detach()[0]
        excess = (log_probs.double() + self.target_entropy).sum()
        rows = float(log_probs.shape[0])
        self.grad_sums.zero_()
        self.grad_sums[0] = -excess
        self.grad_sums[1] = -log_alpha.double() * excess
        self.grad_sums[2] = log_probs.double().sum()
        self.grad_sums[3] = log_alpha.exp() * rows
        self.grad_sums[6] = rows

    def enqueue_step(self, info_row, n_global):
        """log_alpha_t -> log_alpha_{t+1} from the sums of this iteration's actor step; info_row {loss, mean log-prob,
        alpha_t, ...}."""
        self._step(n_global, info_row)

    def enqueue_empty(self, info_row, n_global):
        """This rank drew none of the global batch: zero sums, the same step."""
        self.grad_sums.zero_()
        self._step(n_global, info_row)

    def state_dict(self):
        return {'log_entropy_coeff': self.log_entropy_coeff.detach().cpu().clone()}

    def load_state_dict(self, state):
        self.log_entropy_coeff.copy_(state['log_entropy_coeff'].to(self.log_entropy_coeff.device).reshape(1))
