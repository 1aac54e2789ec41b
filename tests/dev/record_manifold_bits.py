"""Record a golden file of tests/test_gpu_manifold_bits.py: every output array of the named families of the manifold tools' float64
kernels on the test's seeded inputs, with the SHA-256 of every input.  Each family maps to one file (the test's GOLDEN); only the
files of the families given are written, and a file is written whole, so the families that share one are given together.  Needs
an MI355X and the built library; reads nothing outside the repository.  Run it only from a commit whose arithmetic is the one to
pin -- a pull request that changes these kernels' bits on purpose, or one that pins a family for the first time -- and name that
commit in the test's docstring:

    python tests/dev/record_manifold_bits.py [--out-dir DIR] FAMILY [FAMILY ...]
"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import test_gpu_manifold_bits as T  # noqa: E402


def main(families, out_dir):
    unknown = [f for f in families if f not in T.GOLDEN]
    if unknown or not families:
        sys.exit(f"families to record, of {T.FAMILIES}: got {families}")
    for name in sorted({T.GOLDEN[f] for f in families}):
        together = [f for f in T.FAMILIES if T.GOLDEN[f] == name]
        if not set(together) <= set(families):
            sys.exit(f"{name} holds {together}: record them together, or none of them")
        record = {}
        for family in together:
            arrays, hashes = T.compute(family)
            record.update(arrays)
            record.update({k: np.array(v) for k, v in hashes.items()})
            print(f"{family}: {len(arrays)} arrays, {sum(a.nbytes for a in arrays.values())} bytes, {len(hashes)} inputs")
        path = os.path.join(out_dir, name)
        np.savez_compressed(path, **record)
        print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    args = sys.argv[1:]
    out = T.GOLDEN_DIR
    if args[:1] == ["--out-dir"]:
        out, args = args[1], args[2:]
    main(args, out)
