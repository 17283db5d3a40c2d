"""The sha256 of every output buffer of every off-policy entry, at the cases of tests/test_gpu_offpolicy_workspace.py
(seeded inputs; every layout and route of csrc/offpolicy.hip), as one JSON object on stdout.  Two builds of the
library compute the same bits exactly when their outputs here are identical:

    PROBE_LIBRARY=<a libtonic_hip.so> python scripts/offpolicy_entry_bits.py > bits.json

(PROBE_LIBRARY as in scripts/determinism_probe.py; unset: this checkout's library.)  One fresh process per build."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from tonic_amd import _lib   # noqa: E402

if os.environ.get('PROBE_LIBRARY'):            # a variant build of the library (developer)
    _lib.LIBRARY_PATH = os.environ['PROBE_LIBRARY']


def main():
    import test_gpu_offpolicy_workspace as cases
    lib, bits = _lib.load(), {}
    for case in cases.CASES:
        function, kwargs = case.values
        outputs, guard = cases.run_case(lib, function, kwargs)
        assert bool((guard == cases.PATTERN).all()), case.id
        bits[case.id] = {name: hashlib.sha256(tensor.cpu().numpy().tobytes()).hexdigest()
                         for name, tensor in sorted(outputs.items())}
    json.dump(dict(abi=int(lib.tonic_abi_version()), cases=len(bits), sha256=bits), sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
