"""Developer probe: what TD4's twin distributional critics cost beside D4PG and TD3, in one process.

    python scripts/td4_timing.py [--out profiles/td4_timing.json] [--repeats 7]

(PROBE_LIBRARY=<a libtonic_hip.so>: that build of the library, as in scripts/offpolicy_entry_bits.py.)

B = 256, O = 17, A = 6, the agents' default (256, 256) ReLU torsos, 51 atoms, 50 iterations per update call, a full
HBM Buffer of synthetic transitions (as scripts/offpolicy_torso_rate.py fills it).

1. Learner updates/s of TD4, D4PG and TD3 through `agent.enqueue_update` (the captured update graph; TD3 on the
   split entries too, TONIC_AMD_FUSED_ITERATION=0, the route TD4 and D4PG take): a host clock round update calls
   that end in a read-back, the agents taken in turn within each repeat so that drift hits all alike.
2. Device-event time of the two critic entries alone — tonic_twin_distributional_q_grad and
   tonic_distributional_q_grad, no optimizer step — over 200 back-to-back calls captured in one hipGraph.

Median, min and max over the repeats after two warm-up rounds.  The yardstick is D4PG in the same run: the TD4 entry
runs two target forwards, two online forwards and two backwards where D4PG's runs one of each, and shares the
policy pass, so at most twice D4PG's time is what to expect."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tonic_amd import _lib   # noqa: E402

if os.environ.get('PROBE_LIBRARY'):            # a variant build of the library (developer)
    _lib.LIBRARY_PATH = os.environ['PROBE_LIBRARY']

O, A, B, ITERATIONS, ROWS, CALLS, ENTRY_CALLS = 17, 6, 256, 50, 100000, 4, 200


def build(kind):
    import torch
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    replay = tonic_amd.replays.Buffer(size=ROWS, batch_iterations=ITERATIONS, batch_size=B,
                                      return_steps=1 if kind == 'td3' else 5)
    agent = dict(td4=tt.agents.TD4, d4pg=tt.agents.D4PG, td3=tt.agents.TD3)[kind](replay=replay)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    replay._allocate(1, O, A)
    gen = torch.Generator(device=agent.device)
    gen.manual_seed(0)
    for key, buf in replay.buffers.items():
        if key in ('resets', 'terminations'):
            buf.copy_((torch.rand(buf.shape, device=agent.device, generator=gen) < 1e-3).float())
        elif key == 'discounts':
            buf.copy_((1 - replay.buffers['terminations']) * 0.99)
        elif key == 'actions':
            buf.copy_(torch.rand(buf.shape, device=agent.device, generator=gen) * 2 - 1)
        else:
            buf.copy_(torch.randn(buf.shape, device=agent.device, generator=gen))
    replay.size, replay.index = replay.max_size, 0
    return agent


def update_seconds(agent, split):
    """Seconds per update call of ITERATIONS iterations, over CALLS calls that end in a read-back."""
    import torch
    os.environ['TONIC_AMD_FUSED_ITERATION'] = '0' if split else '1'
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        infos = agent.enqueue_update(agent.replay.sample_indices(), agent._draw_noise(ITERATIONS))
    infos.cpu()
    return (time.perf_counter() - t0) / CALLS


def critic_entry(agent, kind):
    """The critic entry of `agent` on one gathered batch as a closure (the updater's own arguments, no step)."""
    import torch
    from tonic_amd import _lib
    u, model, p = agent.critic_updater, agent.model, _lib.ptr
    indices = torch.as_tensor(agent.replay.sample_indices(1)[0], device=agent.device)
    batch = {k: v.clone() for k, v in agent.replay.gather(indices).items()}
    eps = torch.randn(B, A, device=agent.device)
    ws = u._offpolicy_workspace(B)
    mean, std = u.norm_tensors()
    common = (p(model.flat_target_actor.flat), p(model.flat_target_critics.flat), p(u.flat.flat), p(mean), p(std),
              u.norm_clip(), p(batch['observations']), p(batch['actions']), p(batch['next_observations']),
              p(batch['rewards']), p(batch['discounts']))
    shape = (B, u.observation_size, u.hidden, u.action_size, u.atoms)
    if kind == 'td4':
        noise = u.target_action_noise
        name = 'tonic_twin_distributional_q_grad'
        args = common + (p(eps), p(u.values), p(u.grad_sums)) + shape + (float(noise.scale), float(noise.clip))
    else:
        name = 'tonic_distributional_q_grad'
        args = common + (p(u.target_values), p(u.grad_sums)) + shape
    entry = getattr(u.lib, name)
    keep = (batch, eps, ws)

    def call():
        _lib.check(entry(*args, p(ws), ws.numel(), _lib.current_stream()), name)
    call.keep = keep
    return name, call


def captured(call):
    """ENTRY_CALLS calls of the entry back to back in one hipGraph, as the agents' update calls issue them: the
    replay's device time is the kernels' and not the host's launch rate."""
    import torch
    from tonic_amd import _lib
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _lib.capturing(graph):
        for _ in range(ENTRY_CALLS):
            call()
    return graph


def entry_microseconds(graph):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / ENTRY_CALLS


def summary(values):
    return {'median': round(statistics.median(values), 2), 'min': round(min(values), 2),
            'max': round(max(values), 2), 'repeats': len(values)}


def main():
    import torch
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'td4_timing.json'))
    parser.add_argument('--repeats', type=int, default=7)
    options = parser.parse_args()
    assert options.repeats >= 5 and torch.cuda.is_available(), 'needs the GPU and at least 5 repeats'
    # (an agent per route: a captured graph holds the route it was captured on)
    runs = [('td4', 'td4', True), ('d4pg', 'd4pg', True), ('td3_fused', 'td3', False), ('td3_split', 'td3', True)]
    agents = {name: build(kind) for name, kind, _ in runs}
    assert agents['td3_fused']._u.route().fused_kind == 0 and agents['td4']._u.route().fused_kind is None
    entries = dict(critic_entry(agents[kind], kind) for kind in ('td4', 'd4pg'))
    seconds = {name: [] for name, _, _ in runs}
    micros = {name: [] for name in entries}
    graphs = {name: captured(call) for name, call in entries.items()}
    for repeat in range(options.repeats + 2):                  # two warm-up rounds: every shape, every graph
        for name, kind, split in runs:
            dt = update_seconds(agents[name], split)
            if repeat >= 2:
                seconds[name].append(dt)
        for name, graph in graphs.items():
            us = entry_microseconds(graph)
            if repeat >= 2:
                micros[name].append(us)
    result = {'shape': {'B': B, 'O': O, 'A': A, 'torso': [256, 256], 'atoms': 51, 'iterations_per_call': ITERATIONS,
                        'calls_per_repeat': CALLS, 'entry_calls_per_repeat': ENTRY_CALLS},
              'device': torch.cuda.get_device_name(0),
              'learner_updates_per_sec': {name: summary([ITERATIONS / dt for dt in values])
                                          for name, values in seconds.items()},
              'ms_per_update_call': {name: summary([dt * 1e3 for dt in values]) for name, values in seconds.items()},
              'critic_entry_us': {name: summary(values) for name, values in micros.items()}}
    twin, single = (result['critic_entry_us'][name] for name in ('tonic_twin_distributional_q_grad',
                                                                 'tonic_distributional_q_grad'))
    result['critic_entry_ratio_td4_over_d4pg'] = {'of_medians': round(twin['median'] / single['median'], 3),
                                                  'lowest': round(twin['min'] / single['max'], 3),
                                                  'highest': round(twin['max'] / single['min'], 3)}
    os.makedirs(os.path.dirname(os.path.abspath(options.out)), exist_ok=True)
    with open(options.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
