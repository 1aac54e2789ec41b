"""Record tests/golden/manifold_f64_bits.npz: every output array of the manifold tools' float64 kernels on the seeded inputs of
tests/test_gpu_manifold_bits.py, with the SHA-256 of every input.  Needs an MI355X and the built library; reads nothing outside the
repository.  Run it only from a commit whose arithmetic is the one to pin -- a pull request that changes these kernels' bits on
purpose -- and name that commit in the test's docstring:

    python tests/dev/record_manifold_bits.py [output.npz]
"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import test_gpu_manifold_bits as T  # noqa: E402


def main(path):
    record = {}
    for family in T.FAMILIES:
        arrays, hashes = T.compute(family)
        record.update(arrays)
        record.update({k: np.array(v) for k, v in hashes.items()})
        print(f"{family}: {len(arrays)} arrays, {sum(a.nbytes for a in arrays.values())} bytes, {len(hashes)} inputs")
    np.savez_compressed(path, **record)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN)
