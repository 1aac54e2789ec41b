"""One line per case of tests/_launch_trace.matrix(): the SHA-1 of the launch trace ``engine.net_tangent`` makes there (CPU only).

    python tests/dev/net_tangent_trace.py [--tree CHECKOUT] > trace.txt

``--tree``: take the ``cmf_amd`` package from another checkout (a ``git worktree`` of the commit to compare against) with THIS
file's cases and recorders.  Two checkouts make the same launches exactly when their outputs are identical, line for line; the last
line (on stderr) counts the cases and the distinct traces and gives the digest of the whole output."""
import argparse
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(HERE)))
args = ap.parse_args()
sys.path[:0] = [os.path.abspath(args.tree), os.path.dirname(HERE)]

import _launch_trace as LT                     # noqa: E402
from cmf_amd import engine as E                # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(E.__file__))) == os.path.abspath(args.tree), E.__file__
whole, seen, n = hashlib.sha1(), set(), 0
for label, kw, save, tangent, off in LT.matrix():
    d = LT.digest(LT.run(E, kw, save, tangent, off)[1])
    line = f"{label}: {d}\n"
    sys.stdout.write(line)
    whole.update(line.encode())
    seen.add(d)
    n += 1
print(f"{n} cases, {len(seen)} distinct traces, sha1 of the output {whole.hexdigest()}", file=sys.stderr)
