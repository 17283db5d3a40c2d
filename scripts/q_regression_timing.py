"""Developer probe: what tonic_q_regression_grad costs beside the only other route to the same gradient, the DDPG
critic step (tonic_twin_q_grad_loss, kind 2) with rewards = returns and zero discounts, in one process.

    python scripts/q_regression_timing.py [--out profiles/q_regression_timing.json] [--repeats 7]

O = 17, A = 6; the (256, 256) ReLU torso (weight images, one-launch forward and backward) at B = 100, 256 and 1 024,
and one layer-by-layer torso, (400, 300) ReLU, at B = 256.  Device-event time of each entry alone — no optimizer step
— over 200 back-to-back calls captured in one hipGraph, the two entries of a shape replayed alternately within each
repeat so that drift hits both alike.  Median, min and max over the repeats after two warm-up rounds.

The DDPG step runs a target-policy pass, a two-network forward (the target critic beside the online one) and builds
the weight images of three networks where the regression entry encodes, runs one forward and builds one network's
images; the backward chain and the weight-gradient launch are the same.  No ratio is expected in advance: the JSON
holds what was measured."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

O, A, ENTRY_CALLS = 17, 6, 200
SHAPES = [((256, 256), 100), ((256, 256), 256), ((256, 256), 1024), ((400, 300), 256)]


def build(sizes):
    import torch
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    torch.manual_seed(0)
    network = lambda encoder, head: dict(encoder=encoder, torso=tt.models.MLP(sizes, torch.nn.ReLU), head=head)  # noqa: E731
    model = tt.models.ActorCriticWithTargets(
        actor=tt.models.Actor(**network(tt.models.ObservationEncoder(), tt.models.DeterministicPolicyHead())),
        critic=tt.models.Critic(**network(tt.models.ObservationActionEncoder(), tt.models.ValueHead())),
        observation_normalizer=tt.normalizers.MeanStd())
    model.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)))
    model.pack('cuda')
    regression, ddpg = tt.updaters.QRegression(), tt.updaters.DeterministicQLearning()
    regression.initialize(model)
    ddpg.initialize(model)
    assert regression.stock is False and ddpg.stock is False
    return model, regression, ddpg


def entries(model, regression, ddpg, B):
    """The two entries on one batch as closures (the updaters' own arguments, no step)."""
    import torch
    from tonic_amd import _lib
    p = _lib.ptr
    batch = dict(observations=torch.randn(B, O, device='cuda'), actions=torch.rand(B, A, device='cuda') * 2 - 1,
                 next_observations=torch.randn(B, O, device='cuda'), returns=torch.randn(B, device='cuda'),
                 discounts=torch.zeros(B, device='cuda'))
    mean, std = regression.norm_tensors()
    ws = {u: torch.empty(u._offpolicy_workspace(B).numel(), dtype=torch.uint8, device='cuda') for u in (regression, ddpg)}
    sums = {u: torch.zeros_like(u.grad_sums) for u in (regression, ddpg)}
    rule = ctypes.addressof(regression.loss_rule)

    def new():
        w = ws[regression]
        _lib.check(regression.lib.tonic_q_regression_grad(
            p(regression.flat.flat), p(mean), p(std), regression.norm_clip(), p(batch['observations']),
            p(batch['actions']), p(batch['returns']), p(sums[regression]), B, O, regression.hidden, A, rule, None, None,
            p(w), w.numel(), _lib.current_stream()), 'tonic_q_regression_grad')

    def old():
        w = ws[ddpg]
        _lib.check(ddpg.lib.tonic_twin_q_grad_loss(
            2, p(model.flat_target_actor.flat), p(model.flat_target_critics.flat), p(ddpg.flat.flat), p(mean), p(std),
            ddpg.norm_clip(), p(batch['observations']), p(batch['actions']), p(batch['next_observations']),
            p(batch['returns']), p(batch['discounts']), None, p(sums[ddpg]), B, O, ddpg.hidden, A, 0.0, 0.0, 0.0, rule,
            p(w), w.numel(), _lib.current_stream()), 'tonic_twin_q_grad_loss')
    new.keep = old.keep = (batch, ws, sums)
    return {'tonic_q_regression_grad': new, 'tonic_twin_q_grad_loss_kind2_zero_discounts': old}, sums


def captured(call):
    """ENTRY_CALLS calls back to back in one hipGraph: the replay's device time is the kernels', not the host's
    launch rate."""
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
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'q_regression_timing.json'))
    parser.add_argument('--repeats', type=int, default=7)
    options = parser.parse_args()
    assert options.repeats >= 5 and torch.cuda.is_available(), 'needs the GPU and at least 5 repeats'
    models = {sizes: build(sizes) for sizes in {sizes for sizes, _ in SHAPES}}
    result = {'shape': {'O': O, 'A': A, 'entry_calls_per_repeat': ENTRY_CALLS}, 'device': torch.cuda.get_device_name(0),
              'cases': []}
    for sizes, B in SHAPES:
        model, regression, ddpg = models[sizes]
        calls, sums = entries(model, regression, ddpg, B)
        graphs = {name: captured(call) for name, call in calls.items()}
        torch.cuda.synchronize()
        same_bits = bool(torch.equal(sums[regression], sums[ddpg]))        # (the same gradient: what is timed is one job)
        micros = {name: [] for name in graphs}
        for repeat in range(options.repeats + 2):              # two warm-up rounds
            for name, graph in graphs.items():
                us = entry_microseconds(graph)
                if repeat >= 2:
                    micros[name].append(us)
        new, old = (summary(micros[name]) for name in graphs)
        result['cases'].append({
            'torso': list(sizes), 'B': B, 'route': 'images' if sizes[0] == sizes[1] else 'layer by layer',
            'sums_bit_identical': same_bits, 'entry_us': dict(zip(graphs, (new, old))),
            'ratio_regression_over_ddpg_step': {'of_medians': round(new['median'] / old['median'], 3),
                                                'lowest': round(new['min'] / old['max'], 3),
                                                'highest': round(new['max'] / old['min'], 3)}})
    os.makedirs(os.path.dirname(os.path.abspath(options.out)), exist_ok=True)
    with open(options.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
