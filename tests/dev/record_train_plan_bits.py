"""Record tests/golden/train_plan_bits.json on an MI355X: the SHA-1 of every gradient and input cotangent of the six cases of
tests/test_gpu_train_plan.py.  Every case runs twice; a tensor whose two digests differ is listed under ``not_reproducible``.  Run it
only from the commit whose bits are the ones to pin, or against a checkout of that commit, and name the commit in the test's docstring:

    python tests/dev/record_train_plan_bits.py [--tree CHECKOUT] [output.json]

``--tree``: take the ``cmf_amd`` package (built) from another checkout with THIS file's cases."""
import argparse
import json
import os
import sys

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(TESTS))
ap.add_argument("output", nargs="?")
args = ap.parse_args()
sys.path[:0] = [os.path.abspath(args.tree), TESTS]

import cmf_amd  # noqa: E402
import test_gpu_train_plan as T  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(cmf_amd.__file__))) == os.path.abspath(args.tree), cmf_amd.__file__
first, second = T.take_record(), T.take_record()
loose = {case: sorted(n for n in first[case] if first[case][n] != second[case][n]) for case in first}
with open(args.output or T.GOLDEN, "w") as f:
    json.dump({"cases": first, "not_reproducible": {c: n for c, n in loose.items() if n}}, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{os.path.dirname(cmf_amd.__file__)}: {len(first)} cases, not reproducible: {sum(map(len, loose.values()))} tensors")
