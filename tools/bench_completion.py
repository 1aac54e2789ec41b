#!/usr/bin/env python3
"""Cost of the weighted Gauss-Newton step: the one launch of ``engine.weighted_gauss_newton_step`` beside the pair it
stands in for when every weight is one -- ``engine.gram_cholesky(T, d, 1)`` + ``engine.gauss_newton_step`` -- and with a random half
mask beside its own all-ones time, at the head's shapes.

    python tools/bench_completion.py [--reps 30] [--out profiles/completion.txt]

Seeded random panel-layout Jacobian stacks at C3 (B = 512, d = 64, D = 784) and C5 (B = 256, d = 128, D = 3072), random x and x_hat,
damping 1e-3.  HIP events around one launch (around both launches for the pair; the output allocations are inside the bracket,
served by the caching allocator after the warm-up); the variants alternate inside every repetition, so a drift of the machine
reaches all of them alike; median of --reps, and as the run-to-run spread the interquartile range over the median.  Two ratios per
shape:
    (a) weighted launch with unit weights / the pair          -- J read once instead of twice, but the float64 gradient rides on the
                                                                 MFMA pass and only the lower tile triangle is computed
    (b) weighted launch with a half mask / with unit weights  -- the dead rows are not loaded
and the bytes each side has to move, counted from the shapes.  Fails without a GPU."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, reps):
    """{name: [ms per repetition]} of the launches ``fns``, alternated inside every repetition, after three warm-up rounds."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        marks = {}
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            marks[name] = (e0, e1)
        torch.cuda.synchronize()
        for name, (e0, e1) in marks.items():
            ms[name].append(e0.elapsed_time(e1))
    return ms


def spread(v):
    q = statistics.quantiles(v, n=4)
    return (q[2] - q[0]) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "completion.txt"))
    a = ap.parse_args()
    from cmf_amd import engine as E

    assert torch.cuda.is_available(), "bench_completion needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit(f"# weighted step launch (cmf_weighted_gauss_newton_step: G_w by MFMA, g_w and the normal-equation solve in float64, one "
         f"workgroup per sample, J read once) beside the pair gram_cholesky(T, d, 1) + gauss_newton_step (J read twice); HIP events, "
         f"variants alternated, median of {a.reps}, spread = interquartile range / median")
    for label, B, d, D in (("C3", 512, 64, 784), ("C5", 256, 128, 3072)):
        nc = E.ceil16(d)
        T = E.Tangent(B, D, nc, "panel", "cuda", data=(torch.randn(B * D * nc, generator=gen) / D ** 0.5).cuda())
        x, xhat = torch.randn(B, D, generator=gen).cuda(), torch.randn(B, D, generator=gen).cuda()
        lam = torch.full((B,), 1e-3, dtype=torch.float64, device="cuda")
        ones = torch.ones(B, D, device="cuda")
        half = (torch.rand(B, D, generator=gen) < 0.5).float().cuda()
        jtj = E.gram_cholesky(T, d, 1).jtj

        def pair():
            E.gauss_newton_step(T, E.gram_cholesky(T, d, 1).jtj, x, xhat, lam)

        ms = timed({"pair": pair,
                    "gram": lambda: E.gram_cholesky(T, d, 1),
                    "step": lambda: E.gauss_newton_step(T, jtj, x, xhat, lam),
                    "ones": lambda: E.weighted_gauss_newton_step(T, ones, x, xhat, lam, d=d),
                    "half": lambda: E.weighted_gauss_newton_step(T, half, x, xhat, lam, d=d),
                    "cost": lambda: E.weighted_residual_sqnorm(ones, x, xhat)}, a.reps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        r1, rh = E.weighted_gauss_newton_step(T, ones, x, xhat, lam, d=d), E.weighted_gauss_newton_step(T, half, x, xhat, lam, d=d)
        ru = E.gauss_newton_step(T, jtj, x, xhat, lam)
        agree = float(((r1.delta - ru.delta).abs().amax(1) / ru.delta.abs().amax(1)).max())
        bad = int((r1.info != 0).sum()) + int((rh.info != 0).sum())
        live = float(half.sum()) / (B * D)
        mb_j = 4.0 * B * D * nc / 1e6
        emit(f"{label:3s} B = {B:3d} d = {d:3d} D = {D:4d}: pair {med['pair'] * 1e3:7.1f} us (spread {spread(ms['pair']):.3f}; gram_cholesky "
             f"{med['gram'] * 1e3:.1f} + gauss_newton_step {med['step'] * 1e3:.1f}); weighted, unit weights {med['ones'] * 1e3:7.1f} us (spread "
             f"{spread(ms['ones']):.3f}, min {min(ms['ones']) * 1e3:.1f}; {mb_j / med['ones']:.0f} GB/s of the {mb_j:.0f} MB of J); half mask "
             f"({live:.3f} live) {med['half'] * 1e3:7.1f} us (spread {spread(ms['half']):.3f}); cost-only {med['cost'] * 1e3:.1f} us")
        emit(f"    (a) unit weights / pair = {med['ones'] / med['pair']:.3f}   (b) half mask / unit weights = {med['half'] / med['ones']:.3f}"
             f"   bytes of J: pair {2 * mb_j:.0f} MB, weighted {mb_j:.0f} MB, half mask {live * mb_j:.0f} MB; info != 0: {bad}; "
             f"max |delta - pair's delta| / max |delta| = {agree:.2e}")
        del T
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
