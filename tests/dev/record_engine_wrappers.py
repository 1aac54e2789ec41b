"""Record tests/golden/engine_wrappers_host.json: for every call in the tables of tests/test_engine_wrappers_host.py, the exception
type and message of a refused call and the (family, flops, bytes) timer entry of a well-formed one.  Runs on the CPU (no kernel is
launched) and reads nothing outside the repository.  Run it only from the commit whose behaviour is the one to pin, or against a
checkout of that commit, and name the commit in the test's docstring:

    python tests/dev/record_engine_wrappers.py [--tree CHECKOUT] [output.json]

``--tree``: take the ``cmf_amd`` package from another checkout (a ``git worktree`` of the commit to record) with THIS file's tables.
"""
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
import test_engine_wrappers_host as T  # noqa: E402


def main(path):
    record = T.take_record()
    missing = [case for case, r in record["refusals"].items() if r is None]
    assert not missing, f"not refused: {missing}"
    with open(path, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{os.path.dirname(cmf_amd.__file__)}: {len(record['refusals'])} refusals, {len(record['timer'])} timer entries -> {path}")


if __name__ == "__main__":
    main(args.output or T.GOLDEN)
