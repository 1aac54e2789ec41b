#!/usr/bin/env python3
"""Cost of the principal geodesic analysis kernel: ``cmf_tangent_pca`` read with ``engine.timing`` at
(B, K, d) = (16, 64, 128) and (256, 8, 64).

    python tools/bench_tangent_pca.py [--windows 30] [--launches 10] [--out profiles/tangent_pca.txt]

Inputs as in tests/test_gpu_tangent_pca.py: float32 Gram matrices of randn(d + 3, d) with the columns scaled by powers of two
spanning 2^-2 .. 2^2, randn tangent vectors scaled likewise, weights cycled from (1, 2, 0.5, 3, 0.25), all K components.  HIP events
around the launch alone (``engine.timing``; the outputs are allocated by the wrapper outside the events), five launches of warm-up,
then --windows windows of --launches launches each: median, min and max of the windows' mean launch time.  Fails without a GPU."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent_pca.txt"))
    a = ap.parse_args()
    import _tangent_pca_emulation as TE
    from cmf_amd import engine as E

    assert torch.cuda.is_available(), "bench_tangent_pca needs a GPU"
    lines = [f"# cmf_tangent_pca (float64, one workgroup per group, all K components) read with engine.timing: HIP events around the "
             f"launch, median of {a.windows} windows of {a.launches} launches after warm-up"]
    for B, K, d in ((16, 64, 128), (256, 8, 64)):
        G, V, w = (torch.as_tensor(t).cuda() for t in (TE.gram(B, d), TE.vectors(B, K, d), TE.weights(B, K)))
        for _ in range(5):
            r = E.tangent_pca(G, V, w)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.windows):
            with E.timing(lambda name: name == "tangent_pca") as timer:
                for _ in range(a.launches):
                    r = E.tangent_pca(G, V, w)
            n, total, flops, nbytes = timer.by_name()["tangent_pca"]
            ms.append(total / n)
        sweeps = r.sweeps.tolist()
        lines.append(f"(B, K, d) = ({B:3d}, {K:2d}, {d:3d}): tangent_pca {statistics.median(ms) * 1e3:8.1f} us (min {min(ms) * 1e3:.1f}, max "
                     f"{max(ms) * 1e3:.1f}); sweeps {min(sweeps)} .. {max(sweeps)}, info != 0: {int((r.info != 0).sum())}, rank "
                     f"{int(r.rank.min())} .. {int(r.rank.max())}; cost model {flops / n / 1e6:.2f} MFLOP, {nbytes / n / 1e6:.3f} MB per launch")
    print("\n".join(lines), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
