"""TEST INFRASTRUCTURE ONLY — golden vectors of the off-policy agents with torsos of 1 .. 4 layers.

Runs the *unmodified* reference agents (through ``oracle/reference_loader.py``) in the loop of
``oracle/make_golden.run_offpolicy`` with ``torso=(sizes, activation)`` and writes ``tests/golden/<name>.npz``:
SAC / TD3 / DDPG with one, three and four layers, D4PG and MPO with torsos other than two ReLU layers of one
width.  Widths stay at 64 or below (and are not all multiples of 16) so that each fixture is small.

    python scripts/make_torso_goldens.py                  # every fixture, 1 torch thread
    python scripts/make_torso_goldens.py --out DIR NAME   # one fixture, elsewhere (the host test compares)

Needs the reference checkout; the GPU tests read only the committed ``.npz`` files.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import make_golden as mg            # noqa: E402
import reference_loader as rl       # noqa: E402

# name -> (agent kind, run_offpolicy arguments)
CASES = {
    'sac_deep3_small': ('sac', dict(obs_dim=11, act_dim=3, workers=4, batch=24, seed=41,
                                    torso=((64, 48, 32), 'ReLU'))),
    'td3_single_small': ('td3', dict(obs_dim=9, act_dim=4, workers=3, batch=20, seed=42,
                                     torso=((40,), 'Tanh'))),
    'ddpg_deep4_small': ('ddpg', dict(obs_dim=7, act_dim=2, workers=2, batch=16, seed=43,
                                      torso=((32, 32, 24, 16), 'ELU'))),
    'd4pg_uneven_small': ('d4pg', dict(obs_dim=8, act_dim=3, workers=3, batch=20, seed=44, return_steps=3,
                                       torso=((60, 40), 'ReLU'))),
    'd4pg_tanh3_small': ('d4pg', dict(obs_dim=8, act_dim=3, workers=3, batch=20, seed=45, return_steps=3,
                                      torso=((48, 40, 32), 'Tanh'))),
    'mpo_elu_small': ('mpo', dict(obs_dim=9, act_dim=3, workers=3, batch=20, seed=46, return_steps=2,
                                  samples=4, torso=((48, 40), 'ELU'))),
    'mpo_deep3_small': ('mpo', dict(obs_dim=9, act_dim=3, workers=3, batch=20, seed=47, return_steps=2,
                                    samples=4, torso=((40, 32, 24), 'ReLU'))),
}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('names', nargs='*', default=list(CASES))
    parser.add_argument('--out', default=None, help='directory to write to (default tests/golden)')
    args = parser.parse_args()
    torch.set_num_threads(1)
    if args.out:
        mg.OUT = args.out
    tonic = rl.load_reference()
    for name in args.names:
        kind, kwargs = CASES[name]
        mg.run_offpolicy(tonic, name, kind, **kwargs)


if __name__ == '__main__':
    main()
