#!/usr/bin/env python3
"""Cost of the precision guard: the estimator kernel alone at the head's shapes, and a guarded C3 evaluation with no
sample flagged against an unguarded one.

    python tools/bench_guard.py [--reps 20] [--evals 6] [--out FILE]

Kernel: engine.gram_condition on seeded SPD batches (C3 B = 512 d = 64, C5 B = 256 d = 128, d = 512 B = 8), HIP events around
each launch pair (condition + flag list) after warm-up, median of --reps.  End to end: full-size C3 (recipe seed 0), B = 512
seeded inputs, ``elbo(add_offdiagonal_metric_reg=True)`` under no_grad, host clock around each call ending in a synchronise,
guarded (default PrecisionGuard; nothing must be flagged, checked) and unguarded calls alternated, medians of --evals each.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spd_batch(B, d, gen):
    j = torch.randn(B, 2 * d, d, generator=gen) / (2 * d) ** 0.5
    return (j.transpose(1, 2) @ j + 0.1 * torch.eye(d)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--evals", type=int, default=6)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict

    assert torch.cuda.is_available(), "bench_guard needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit("# estimator kernel (cmf_gram_condition: float64 condition numbers + flag list), median of %d launches" % a.reps)
    for label, B, d in (("C3", 512, 64), ("C5", 256, 128), ("d512", 8, 512)):
        r = E.GramResult()
        r.jtj = spd_batch(B, d, gen).cuda()
        r.info = torch.zeros(B, dtype=torch.int32, device="cuda")
        for _ in range(3):
            E.gram_condition(r, d, 1e4)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            E.gram_condition(r, d, 1e4)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        emit(f"{label:5s} B = {B:3d} d = {d:3d}: {statistics.median(ms) * 1e3:9.1f} us  (min {min(ms) * 1e3:.1f}, "
             f"{statistics.median(ms) * 1e3 / B:.2f} us per sample)")

    cfg = cmf_amd.get_config("mnist", latent_dimension=64, log_jacobian_method="cholesky")
    schema = cmf_amd.get_schema(cfg)
    B = a.batch
    x = torch.randint(0, 256, (B, 1, 28, 28), generator=gen).float() + torch.rand(B, 1, 28, 28, generator=gen)
    dens = cmf_amd.get_density(schema, x[:2])
    dens.load_state_dict(fill_state_dict(dens.state_dict(), seed=0))
    dens = dens.cuda().eval()
    model = dens.module.density
    head = next(m for m in dens.modules() if type(m).__name__ == "NonSquareHeadDensity")
    xc = x.cuda()
    guard = cmf_amd.PrecisionGuard()

    def run(g):
        head.precision_guard = g
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = model.elbo(xc, add_offdiagonal_metric_reg=True)["elbo"]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    run(None), run(guard)
    times = {None: [], guard: []}
    outs = {}
    for _ in range(a.evals):
        for g in (None, guard):
            ms, outs[g] = run(g)
            times[g].append(ms)
    flagged = int(head.last_gram.flagged_count.item())
    same = torch.equal(outs[None], outs[guard])
    cmax = float(head.last_gram.cond.max())
    t_plain, t_guard = statistics.median(times[None]), statistics.median(times[guard])
    emit(f"# C3 full size, B = {B}, elbo(add_offdiagonal_metric_reg=True), median of {a.evals} alternated calls each")
    emit(f"unguarded {t_plain:8.2f} ms  ({sorted(round(t, 2) for t in times[None])})")
    emit(f"guarded   {t_guard:8.2f} ms  ({sorted(round(t, 2) for t in times[guard])})  max_condition {guard.max_condition:.3g}, "
         f"flagged {flagged}, max cond {cmax:.3e}, elbo bit-equal {same}")
    emit(f"overhead  {100.0 * (t_guard - t_plain) / t_plain:+.2f} %")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
