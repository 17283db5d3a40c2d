"""profiles/lr_schedule_timing.json: what a learning-rate schedule costs on the HIP optimizer steps.

Device-event medians over 7 replays of a captured graph of 200 calls, two fresh processes per figure, the builds (or
the scheduled / unscheduled forms) alternating; every case is a process of its own under a time limit (this script
calling itself with `--case`) and the driver stops at the first case that fails.  There is no fallback: without a GPU
the first case fails and so does the script.

    step         tonic_optimizer_step at n = 4 194 304 and 70 000, unscheduled, this build against `--baseline
                 other/libtonic_hip.so` (a build of the parent commit): the kernels are unchanged, the difference is
                 to lie inside the parent's own window spread
    scheduled    tonic_scheduled_optimizer_step against tonic_optimizer_step on this build at both sizes, Adam under
                 COSINE and SGD under EXPONENTIAL (recorded; no threshold)
    pair         a PPO iteration's step (actor 5 708, critic 5 377 parameters) through tonic_scheduled_adam_step_pair
                 against tonic_adam_step_pair
    sac          one fused SAC iteration at B = 256 and 1 024 with the warm-up + cosine schedule on both updaters
                 against none (the same launches with other table values), and the route the scheduled agent takes

`python scripts/lr_schedule_timing.py [output.json] --baseline other/libtonic_hip.so`"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
CALLS, REPLAYS, WARM, SIZES, LIMIT = 200, 7, 3, (4_194_304, 70_000), 180
SAC_ITERATIONS = 10


def replays_us(graph, per):
    """Device-event time of each of REPLAYS replays (after WARM) divided by `per`, in microseconds."""
    import torch
    times = []
    for i in range(WARM + REPLAYS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            times.append(a.elapsed_time(b) * 1e3 / per)
    return times


def captured(step):
    import torch
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'lr_schedule_timing.py needs the GPU'
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _lib.capturing(graph):
        for _ in range(CALLS):
            step()
    return graph


def case_step(n, rule_name, schedule_name, library):
    import ctypes
    import numpy as np
    import torch
    import lr_schedule_ref as sref
    import optim_family_ref as ref
    from tonic_amd import _lib
    from tonic_amd.torch import updaters
    lib = _lib.load()
    rng = np.random.RandomState(n % 65521)
    dev = lambda a: torch.as_tensor(np.asarray(a, np.float32)).cuda()                  # noqa: E731
    params, sums = dev(rng.normal(size=n)), dev(np.concatenate([rng.normal(size=n) * 37, np.zeros(8)]))
    state = torch.tensor([5, 0, 0, 0], dtype=torch.int32, device='cuda')
    factory = (lambda p: torch.optim.Adam(p, lr=3e-4)) if rule_name == 'adam' else ref.factory(rule_name)
    packed, buffers = updaters.optimizer_slots(lib, updaters.optimizer_hyperparameters(factory, 1e-3), n, 'cuda')
    schedule = sref.pack(sref.SCHEDULES[schedule_name][1]) if schedule_name != 'none' else None
    entry = lib.tonic_optimizer_step
    if library != 'this':
        foreign = ctypes.CDLL(library)
        entry = foreign.tonic_optimizer_step
        entry.restype, entry.argtypes = _lib.SIGNATURES['tonic_optimizer_step']
    tail = ()
    if schedule is not None:
        entry, tail = lib.tonic_scheduled_optimizer_step, (ctypes.byref(schedule),)

    def step():
        status = entry(params.data_ptr(), sums.data_ptr(), _lib.ptr(buffers), state.data_ptr(), n, 1.0 / 37,
                       ctypes.byref(packed), 0, 0.0, 0.0, None, None, None, None, None, 0, 0, 0.0, *tail,
                       _lib.current_stream())
        assert status == 0, lib.tonic_last_error()
    times = replays_us(captured(step), CALLS)
    assert int(state[0]) == 5 + 1 + CALLS * (WARM + REPLAYS) and bool(torch.isfinite(params).all())
    return times


def case_pair(form):
    import ctypes
    import numpy as np
    import torch
    import lr_schedule_ref as sref
    from tonic_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(7)
    dev = lambda a: torch.as_tensor(np.asarray(a, np.float32)).cuda()                  # noqa: E731
    nets = []
    for n in (lib.tonic_ppo_actor_param_count(17, 6), lib.tonic_v_critic_param_count(17)):
        nets.append(dict(n=n, p=dev(rng.normal(size=n)), sums=dev(np.concatenate([rng.normal(size=n), np.zeros(8)])),
                         m=dev(np.zeros(n)), v=dev(np.zeros(n)), info=dev(np.zeros(8)),
                         state=torch.zeros(4, dtype=torch.int32, device='cuda')))
    a, c = nets
    adv = dev([0.0, 1.0, 0.0, 0.0])
    schedule = sref.pack(sref.SCHEDULES['warmup-cosine'][1])
    entry, tail = lib.tonic_adam_step_pair, ()
    if form == 'scheduled':
        entry, tail = lib.tonic_scheduled_adam_step_pair, (ctypes.byref(schedule), ctypes.byref(schedule))
    q = lambda t: t.data_ptr()                                                          # noqa: E731

    def step():
        status = entry(q(a['p']), q(a['sums']), q(a['m']), q(a['v']), q(a['state']), a['n'], 3e-4, 1, 1e9, 0.0, q(adv),
                       q(a['info']), None, q(c['p']), q(c['sums']), q(c['m']), q(c['v']), q(c['state']), c['n'], 1e-3,
                       2, q(c['info']), 1.0 / 64, 0.9, 0.999, 1e-8, *tail, _lib.current_stream())
        assert status == 0, lib.tonic_last_error()
    times = replays_us(captured(step), CALLS)
    assert int(a['state'][0]) == int(c['state'][0]) == 1 + CALLS * (WARM + REPLAYS)
    return times


def case_sac(B, form):
    import numpy as np
    import torch
    import lr_schedule_ref as sref
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    assert torch.cuda.is_available(), 'lr_schedule_timing.py needs the GPU'
    O, A, W, rows = 17, 6, 4, 600
    scheduler = sref.factory('warmup-cosine') if form == 'scheduled' else None
    agent = tt.agents.SAC(
        replay=tonic_amd.replays.Buffer(size=rows * W, batch_iterations=SAC_ITERATIONS, batch_size=B,
                                        steps_before_batches=0, steps_between_batches=1),
        actor_updater=tt.updaters.TwinCriticSoftDeterministicPolicyGradient(lr_scheduler=scheduler),
        critic_updater=tt.updaters.TwinCriticSoftQLearning(lr_scheduler=scheduler))
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=7)
    rng = np.random.RandomState(321)
    for _ in range(rows - 3):
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, size=(W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        agent.replay.store(normalizer=agent.model.observation_normalizer,
                           **{k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in row.items()})
    route = agent._u.route()
    assert route.fused_kind == 1 and not route.in_phases, 'the scheduled SAC agent left the fused iteration'
    times = []
    for i in range(WARM + REPLAYS):
        indices = rng.randint(0, agent.replay.size * agent.replay.global_workers,
                              size=(SAC_ITERATIONS, B)).astype(np.int64)
        eps = rng.normal(size=agent._draw_noise(SAC_ITERATIONS).shape).astype(np.float32)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        # (the host's uploads of this call's streams are enqueued ahead of the first event)
        slot = agent._u._prepare(indices, eps)
        if slot.graph is None:
            agent.enqueue_update(indices, eps)
            torch.cuda.synchronize()
            continue
        agent._u._upload_adam_table(slot, [bool(agent._actor_due(it)) for it in range(SAC_ITERATIONS)])
        torch.cuda.synchronize()
        a.record()
        slot.graph.replay()
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            times.append(a.elapsed_time(b) * 1e3 / SAC_ITERATIONS)
    assert bool(torch.isfinite(agent.model.flat_online).all())
    agent.close()
    return times, 'fused (tonic_q_iteration, kind 1)'


def case(arguments):
    kind = arguments[0]
    if kind == 'step':
        out = dict(replays_us=case_step(int(arguments[1]), arguments[2], arguments[3], arguments[4]))
    elif kind == 'pair':
        out = dict(replays_us=case_pair(arguments[1]))
    else:
        times, route = case_sac(int(arguments[1]), arguments[2])
        out = dict(replays_us=times, route=route)
    print(json.dumps(out))


def figure(variants):
    """{name: case arguments} -> {name: median, window over both processes' replays}; the variants alternate."""
    import numpy as np
    runs = {name: [] for name in variants}
    extra = {}
    for _ in range(2):
        for name, arguments in variants.items():
            done = subprocess.run([sys.executable, os.path.abspath(__file__), '--case'] + [str(a) for a in arguments],
                                  capture_output=True, text=True, timeout=LIMIT)
            if done.returncode != 0:
                sys.exit(f'{name} {arguments}: exit status {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}')
            result = json.loads(done.stdout.strip().splitlines()[-1])
            runs[name].append(result.pop('replays_us'))
            extra.setdefault(name, {}).update(result)
    out = {}
    for name, (first, second) in runs.items():
        both = np.array(first + second)
        out[name] = dict(median_us=round(float(np.median(both)), 3),
                         process_medians_us=[round(float(np.median(first)), 3), round(float(np.median(second)), 3)],
                         window_us=[round(float(both.min()), 3), round(float(both.max()), 3)], **extra[name])
    return out


def main(arguments):
    if arguments[:1] == ['--case']:
        return case(arguments[1:])
    if '--baseline' not in arguments:
        sys.exit('lr_schedule_timing.py: --baseline path/to/the/parent/libtonic_hip.so is needed')
    at = arguments.index('--baseline')
    baseline = os.path.abspath(arguments[at + 1])
    del arguments[at:at + 2]
    target = arguments[0] if arguments else os.path.join(ROOT, 'profiles', 'lr_schedule_timing.json')
    out = dict(calls_per_graph=CALLS, replays=REPLAYS, processes_per_figure=2, unit='microseconds per call',
               unscheduled_step={}, scheduled_step={}, ppo_pair={}, sac_iteration={})
    for n in SIZES:
        out['unscheduled_step'][str(n)] = figure({'parent': ('step', n, 'adam', 'none', baseline),
                                                  'this': ('step', n, 'adam', 'none', 'this')})
        out['scheduled_step'][str(n)] = figure({
            'adam': ('step', n, 'adam', 'none', 'this'), 'adam under cosine': ('step', n, 'adam', 'cosine', 'this'),
            'sgd': ('step', n, 'sgd', 'none', 'this'),
            'sgd under exponential': ('step', n, 'sgd', 'exponential', 'this')})
    out['ppo_pair'] = figure({'plain': ('pair', 'plain'), 'scheduled': ('pair', 'scheduled')})
    for B in (256, 1024):
        out['sac_iteration'][str(B)] = figure({'unscheduled': ('sac', B, 'plain'), 'scheduled': ('sac', B, 'scheduled')})
    with open(target, 'w') as handle:
        json.dump(out, handle, indent=1)
        handle.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1:])
