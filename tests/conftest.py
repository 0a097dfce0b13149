import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")

# Test infrastructure only: the torch modules of oracle/ that the three-way tests run ON THE DEVICE (fp64 / fp32 replays of the product's
# branch) go through MIOpen, whose default exhaustive "find" benchmarks every applicable solver the first time it meets a convolution
# configuration -- on a fresh box (empty ~/.cache/miopen) that is 94 s for two of these tests against 28 s with the heuristic pick.
# The product's own kernels never touch MIOpen.
os.environ.setdefault("MIOPEN_FIND_MODE", "2")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: CPU oracle at full size (tens of seconds each; still part of -m 'not gpu')")


class GoldenParts:
    """One fixture stored as ``<name>.npz`` plus ``<name>.part1.npz``, ``<name>.part2.npz``, ... (no committed file over 1 MiB):
    the arrays of all parts under one ``.files`` / ``[key]`` interface, as ``np.load`` of a single file gives them."""

    def __init__(self, parts):
        self._parts = parts
        self.files = [k for p in parts for k in p.files]

    def __getitem__(self, key):
        for p in self._parts:
            if key in p.files:
                return p[key]
        raise KeyError(key)

    def __contains__(self, key):
        return key in self.files

    def __iter__(self):
        return iter(self.files)


@pytest.fixture(scope="session")
def golden():
    import numpy as np

    def load(name):
        parts = [np.load(os.path.join(GOLDEN, name + ".npz"))]
        while os.path.exists(os.path.join(GOLDEN, f"{name}.part{len(parts)}.npz")):
            parts.append(np.load(os.path.join(GOLDEN, f"{name}.part{len(parts)}.npz")))
        return parts[0] if len(parts) == 1 else GoldenParts(parts)
    return load
