"""profiles/trpo_hip_timing.json: one Fisher-vector product and one whole TRPO actor step, the stock autograd path
(TONIC_AMD_TRPO_HIP=0: the code before the tonic_trpo_* entries) then the HIP path, in the same process order at each
size; HalfCheetah shapes, default torso; device events over 20 repetitions after 3 warm-up ones.
`python scripts/trpo_hip_timing.py [output.json]`"""
import json
import os
import sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from test_gpu_trpo_hip import step_problem          # noqa: E402
from tonic_amd import _lib                          # noqa: E402
from tonic_amd.torch import updaters                # noqa: E402

REPS, WARM = 20, 3


def timed(fn, before=None):
    times = []
    for i in range(WARM + REPS):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            times.append(a.elapsed_time(b))
    t = np.array(times)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), reps=REPS)


out = dict(device=torch.cuda.get_device_name(0), shapes=dict(O=17, A=6, torso=[64, 64]), sizes={})
for n in (262144, 1048576):
    row = {}
    for switch, name in (('0', 'stock'), ('1', 'hip')):
        os.environ['TONIC_AMD_TRPO_HIP'] = switch
        model, batch = step_problem(5, 1.0, n=n)
        model.pack('cuda')
        up = updaters.TrustRegionPolicyGradient()
        up.initialize(model)
        assert up.hip is (switch == '1')
        b = {k: torch.as_tensor(v).cuda() for k, v in batch.items()}
        flat = model.flat_actor.flat
        start = flat.clone()
        v = torch.randn(flat.numel(), device='cuda')
        if switch == '0':
            with torch.no_grad():
                beh = model.actor(b['observations'])
                locs, scales = beh.loc, beh.stddev
            variables = up.variables

            def fvp():
                first = torch.cat([t.reshape(-1) for t in torch.autograd.grad(
                    up._kl(b['observations'], locs, scales), variables, create_graph=True)])
                return torch.cat([t.reshape(-1) for t in torch.autograd.grad((first * v).sum(), variables)])
        else:
            lib, ws = up.lib, up._hip_workspace_for(n)
            sums = torch.empty(flat.numel() + 8, device='cuda')
            _lib.check(lib.tonic_trpo_prepare(*up.hip_torso, flat.data_ptr(), b['observations'].data_ptr(), n, 17, 6,
                                              None, None, ws.data_ptr(), ws.numel(), _lib.current_stream()), 'prepare')

            def fvp():
                _lib.check(lib.tonic_trpo_fisher_vector(*up.hip_torso, flat.data_ptr(), b['observations'].data_ptr(),
                                                        v.data_ptr(), sums.data_ptr(), n, 17, 6, ws.data_ptr(),
                                                        ws.numel(), _lib.current_stream()), 'fvp')
        row[name + '_fvp'] = timed(fvp)
        result = {}

        def step():
            result.update(up(**b))
        row[name + '_step'] = timed(step, before=lambda: flat.copy_(start))
        row[name + '_step']['backtrack_steps'] = int(result['backtrack_steps'])
        row[name + '_step']['kl'] = float(result['kl'])
        print(n, name, row[name + '_fvp'], row[name + '_step'], flush=True)
        del up, model, b
        torch.cuda.empty_cache()
    traffic = 4 * n * (2 * 17 + 6 * (64 + 64) + 6 * 6)
    row['fvp_algorithmic_bytes'] = traffic
    row['fvp_algorithmic_bytes_formula'] = ('4 n (2 O + 6 sum(H) + 6 A): x read by the first tangent layer and by dW1; '
                                            'every h_l read by both passes; tangents, hidden gradients, mu and the '
                                            'head rows written once and read once')
    row['hip_fvp_bytes_per_s'] = traffic / (row['hip_fvp']['median_ms'] * 1e-3)
    row['fvp_speedup'] = row['stock_fvp']['median_ms'] / row['hip_fvp']['median_ms']
    row['step_speedup'] = row['stock_step']['median_ms'] / row['hip_step']['median_ms']
    out['sizes'][str(n)] = row
target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'trpo_hip_timing.json')
json.dump(out, open(target, 'w'), indent=1)
print(json.dumps(out))
