"""Developer probe (profiles/collect_host_window.md): the collect loop of the bench workload (256 workers, O = 17,
A = 6) on the tree's library or on another build's (the parent commit's, say): microseconds per environment step
over `rounds` x 2048 steps, then where 3000 steps go (agent.step / environment.step / agent.update, and the time
blocked in tonic_collector_wait_actions).  One build per process: alternate the processes on one box.
usage: collect_host_window.py [rounds] [--library PATH/libtonic_hip.so]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tonic_amd import _lib
arguments = sys.argv[1:]
if '--library' in arguments:
    at = arguments.index('--library')
    _lib.LIBRARY_PATH = os.path.abspath(arguments[at + 1])
    del arguments[at:at + 2]
import numpy as np, torch
import bench
from tonic_amd.utils import logger
logger.get_current_logger().store = lambda *a, **k: None
rounds = int(arguments[0]) if arguments else 4


def between_rollouts(agent, loop):
    loop.run(bench.T - agent.replay.index)             # finish the segment: a learner update
    agent.settle()
    torch.cuda.synchronize()
    loop.run(64)


agent, loop, rollout, out = bench.measure_job(256, 0, 1, 1, 0, True, device_too=False)
times = []
for r in range(rounds):
    between_rollouts(agent, loop)
    t0 = time.perf_counter()
    loop.run(2048)
    times.append((time.perf_counter() - t0) / 2048 * 1e6)
between_rollouts(agent, loop)
collector, blocked = agent._rollout.collector, [0.0]
wait = collector._wait


def timed(*args):
    t0 = time.perf_counter()
    status = wait(*args)
    blocked[0] += time.perf_counter() - t0
    return status


collector._wait = timed
parts = loop.breakdown(3000)
collector._wait = wait
print(json.dumps(dict(library=_lib.LIBRARY_PATH, us_per_env_step=[round(t, 3) for t in times],
                      median=round(float(np.median(times)), 3), transport=agent.transport_in_effect,
                      breakdown={k: parts[k] for k in ('us_per_env_step', 'agent_step_us', 'env_step_us',
                                                       'agent_update_us')},
                      wait_us=round(blocked[0] / 3000 * 1e6, 3))))
agent.close()
