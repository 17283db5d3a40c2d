"""profiles/optim_family_timing.json: tonic_optimizer_step per rule of the optimizer family against tonic_adam_step, at
n = 98 311 (three grid-stride passes, launch-bound) and n = 4 194 304 (HBM-bound: the expectation is the ratio of bytes
per parameter, 12 + 8 per state buffer against Adam's 28).  Device events over 50 repetitions after 5 warm-up ones.

Every case is a process of its own under a time limit (this script calling itself with `--case`); the driver stops at the
first case that fails.  `python scripts/optim_family_timing.py [output.json] [--baseline other/libtonic_hip.so]`: with
`--baseline`, tonic_adam_step of that library (a build of the parent commit) is timed beside this one's."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
REPS, WARM, SIZES, LIMIT = 50, 5, (98_311, 4_194_304), 120


def case(name, n, library):
    import ctypes
    import numpy as np
    import torch
    import optim_family_ref as ref
    from tonic_amd import _lib
    from tonic_amd.torch import updaters
    lib = _lib.load()
    rng = np.random.RandomState(n % 65521)
    dev = lambda a: torch.as_tensor(np.asarray(a, np.float32)).cuda()                  # noqa: E731
    params, sums = dev(rng.normal(size=n)), dev(np.concatenate([rng.normal(size=n) * 37, np.zeros(8)]))
    state = torch.tensor([5, 0, 0, 0], dtype=torch.int32, device='cuda')
    if name == 'adam':
        if library:
            lib = ctypes.CDLL(library)
            lib.tonic_adam_step.restype, lib.tonic_adam_step.argtypes = _lib.SIGNATURES['tonic_adam_step']
        m, v = dev(np.zeros(n)), dev(np.zeros(n))
        slots, per_parameter = 2, 28

        def step():
            status = lib.tonic_adam_step(params.data_ptr(), sums.data_ptr(), m.data_ptr(), v.data_ptr(),
                                         state.data_ptr(), n, 1.0 / 37, 3e-4, 0.9, 0.999, 1e-8, 0, 0.0, 0.0, None, None,
                                         None, None)
            assert status == 0
    else:
        rule = updaters.optimizer_hyperparameters(ref.factory(name), 1e-3)
        packed, buffers = updaters.optimizer_slots(lib, rule, n, 'cuda')
        slots = len(ref.slot_names(rule))
        per_parameter = 12 + 8 * slots

        def step():
            _lib.check(lib.tonic_optimizer_step(
                params.data_ptr(), sums.data_ptr(), _lib.ptr(buffers), state.data_ptr(), n, 1.0 / 37,
                ctypes.byref(packed), 0, 0.0, 0.0, None, None, None, None, None, 0, 0, 0.0, None),
                'tonic_optimizer_step')
    times = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); step(); b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            times.append(a.elapsed_time(b) * 1e3)
    t = np.array(times)
    assert int(state[0]) == 5 + WARM + REPS and bool(torch.isfinite(params).all())
    print(json.dumps(dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()), reps=REPS,
                          state_buffers=slots, bytes_per_parameter=per_parameter)))


def main(arguments):
    if arguments[:1] == ['--case']:
        return case(arguments[1], int(arguments[2]), arguments[3] if len(arguments) > 3 else None)
    import optim_family_ref as ref
    baseline = None
    if '--baseline' in arguments:
        at = arguments.index('--baseline')
        baseline = os.path.abspath(arguments[at + 1])
        del arguments[at:at + 2]
    target = arguments[0] if arguments else os.path.join(ROOT, 'profiles', 'optim_family_timing.json')
    out = dict(reps=REPS, warmup=WARM, sizes={})
    for n in SIZES:
        rows = {}
        cases = [('adam', None)] + ([('adam (baseline library)', baseline)] if baseline else []) + \
            [(name, None) for name in ref.CONFIGURATIONS]
        for name, library in cases:
            command = [sys.executable, os.path.abspath(__file__), '--case', name.split(' ')[0], str(n)] + \
                ([library] if library else [])
            done = subprocess.run(command, capture_output=True, text=True, timeout=LIMIT)
            if done.returncode != 0:
                sys.exit(f'{name} at n = {n} ended with status {done.returncode}:\n{done.stdout}\n{done.stderr}')
            rows[name] = json.loads(done.stdout.strip().split('\n')[-1])
            print(n, name, rows[name], flush=True)
        adam = rows['adam']
        for name, row in rows.items():
            row['time_over_adam'] = row['median_us'] / adam['median_us']
            row['bytes_over_adam'] = row['bytes_per_parameter'] / adam['bytes_per_parameter']
            row['bytes_per_s'] = row['bytes_per_parameter'] * n / (row['median_us'] * 1e-6)
        out['sizes'][str(n)] = rows
    json.dump(out, open(target, 'w'), indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1:])
