"""One line per case and pass of tests/_launch_trace.train_matrix(): the SHA-1 of the launch trace ``engine.net_primal``,
``engine.net_tangent(save=)``, ``engine.net_cotangent`` and ``engine.net_primal_backward`` make there (CPU only).

    python tests/dev/train_trace.py [--tree CHECKOUT] [--golden FILE] > trace.txt

``--tree``: take the ``cmf_amd`` package from another checkout (a ``git worktree`` of the commit to compare against) with THIS
file's cases and recorders.  Two checkouts make the same launches exactly when their outputs are identical, line for line; the last
line (on stderr) counts the cases and the distinct traces and gives the digest of the whole output.  ``--golden FILE``: write the
digests of tests/_launch_trace.train_subset() there instead (tests/golden/train_trace.json, read by tests/test_train_plan_host.py);
record it with ``--tree`` at the commit whose launches are the ones to pin, and name that commit in the test's docstring."""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(HERE)))
ap.add_argument("--golden")
args = ap.parse_args()
sys.path[:0] = [os.path.abspath(args.tree), os.path.dirname(HERE)]

import _launch_trace as LT                     # noqa: E402
from cmf_amd import engine as E                # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(E.__file__))) == os.path.abspath(args.tree), E.__file__
if args.golden:
    record = {label: {p: LT.digest(r) for p, r in LT.run_train(E, **kw).items()} for label, kw in LT.train_subset()}
    with open(args.golden, "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{os.path.dirname(E.__file__)}: {len(record)} cases -> {args.golden}", file=sys.stderr)
    sys.exit(0)
whole, seen, n = hashlib.sha1(), set(), 0
for label, kw in LT.train_matrix():
    for p, r in LT.run_train(E, **kw).items():
        d = LT.digest(r)
        line = f"{label} {p}: {d}\n"
        sys.stdout.write(line)
        whole.update(line.encode())
        seen.add(d)
    n += 1
print(f"{n} cases, {len(seen)} distinct traces, sha1 of the output {whole.hexdigest()}", file=sys.stderr)
