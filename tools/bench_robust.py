#!/usr/bin/env python3
"""Cost of the robust projection: the ``engine.robust_weights`` launch -- exact median, weights, robust cost -- beside
``engine.weighted_residual_sqnorm``, the cost-only launch of ``complete`` it replaces in the loop, and one
``ManifoldProjector.robust(steps=4)`` against ``complete(steps=4)`` with unit weights on the same input, on the full-size C3 model.

    python tools/bench_robust.py [--reps 30] [--evals 6] [--out profiles/robust.txt] [--launches-only]

Kernel: seeded random x and x_hat at C3 (B = 512, D = 784) and C5 (B = 256, D = 3072), unit prior weights on the side of
``weighted_residual_sqnorm``, no prior on the side of ``robust_weights`` (what ``robust`` passes when the caller gives no weights).
HIP events around one launch (the output allocations are inside the bracket, served by the caching allocator after the warm-up),
median of --reps after three warm-up launches, for: the estimating mode (scale_in NULL: the validating pass, seven more select
passes, the weights pass), the held-scale mode the loop runs in (two passes), its cost-only variant, and both losses.  The byte
figure is the one the engine's timer entry counts (every pass's reads; only the first comes from HBM).  End to end: full-size C3
(recipe seed 0), B = 512 seeded inputs past the dequantisation wrapper, host clock around work that ends in a synchronise, alternated,
medians of --evals; both calls run the same number of launches per iteration.  Fails without a GPU."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--evals", type=int, default=6)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust.txt"))
    ap.add_argument("--launches-only", action="store_true", help="the launch table alone, nothing written: what a kernel trace runs")
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict

    assert torch.cuda.is_available(), "bench_robust needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit(f"# robust weights launch (cmf_robust_weights: exact lower median of |x - xhat| by an 8-pass radix select, IRLS weights and "
         f"robust cost in float64, one workgroup per sample) beside weighted_residual_sqnorm (the cost-only launch of complete); HIP "
         f"events, median of {a.reps}")
    for label, B, D in (("C3", 512, 784), ("C5", 256, 3072)):
        x, xhat = torch.randn(B, D, generator=gen).cuda(), torch.randn(B, D, generator=gen).cuda()
        ones = torch.ones(B, D, device="cuda")
        r = E.robust_weights(x, xhat, "huber", 1.345)
        scale = r.scale.contiguous()
        with E.timing(lambda name: name == "robust_weights") as timer:
            E.robust_weights(x, xhat, "huber", 1.345)
            E.robust_weights(x, xhat, "huber", 1.345, scale=scale)
        by_est, by_held = (rec[2] for rec in timer.records)             # (name, flops, bytes, event, event) per launch
        m = {}
        m["estimate"] = event_ms(lambda: E.robust_weights(x, xhat, "huber", 1.345), a.reps)
        m["held"] = event_ms(lambda: E.robust_weights(x, xhat, "huber", 1.345, scale=scale), a.reps)
        m["held, tukey"] = event_ms(lambda: E.robust_weights(x, xhat, "tukey", 4.685, scale=scale), a.reps)
        m["held, cost only"] = event_ms(lambda: E.robust_weights(x, xhat, "huber", 1.345, scale=scale, weights_out=False), a.reps)
        m["sqnorm"] = event_ms(lambda: E.weighted_residual_sqnorm(ones, x, xhat), a.reps)
        med = {k: statistics.median(v) for k, v in m.items()}
        emit(f"{label:3s} B = {B:3d} D = {D:4d}: robust_weights estimating {med['estimate'] * 1e3:7.1f} us (min "
             f"{min(m['estimate']) * 1e3:.1f}; {by_est / 1e6:.1f} MB counted = {by_est / med['estimate'] / 1e6:.0f} GB/s); held scale "
             f"{med['held'] * 1e3:7.1f} us (min {min(m['held']) * 1e3:.1f}; {by_held / 1e6:.1f} MB = {by_held / med['held'] / 1e6:.0f} GB/s), "
             f"tukey {med['held, tukey'] * 1e3:7.1f} us, cost only {med['held, cost only'] * 1e3:7.1f} us; weighted_residual_sqnorm "
             f"{med['sqnorm'] * 1e3:7.1f} us (min {min(m['sqnorm']) * 1e3:.1f}): held x {med['held'] / med['sqnorm']:.2f}, estimating x "
             f"{med['estimate'] / med['sqnorm']:.2f}; info != 0: {int((r.info != 0).sum())}")
    if a.launches_only:
        return

    cfg = cmf_amd.get_config("mnist", latent_dimension=64, log_jacobian_method="cholesky")
    B = a.batch
    x = torch.randint(0, 256, (B, 1, 28, 28), generator=gen).float() + torch.rand(B, 1, 28, 28, generator=gen)
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), x[:2])
    dens.load_state_dict(fill_state_dict(dens.state_dict(), seed=0))
    dens = dens.cuda().eval()
    model = dens.module.density                     # past the dequantisation wrapper: both sides see the same input
    proj = cmf_amd.ManifoldProjector(model, steps=4)
    xc = x.cuda()
    ones = torch.ones_like(xc)
    last = {}

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    runners = {"complete(steps=4)": lambda: last.__setitem__("complete", proj.complete(xc, ones)),
               "robust(steps=4)": lambda: last.__setitem__("robust", proj.robust(xc)),
               "robust(steps=4, tukey)": lambda: last.__setitem__("tukey", proj.robust(xc, loss="tukey")),
               "robust(steps=2, rounds=2)": lambda: last.__setitem__("rounds", proj.robust(xc, steps=2, rounds=2))}
    for fn in runners.values():
        run(fn)
        run(fn)
    times = {which: [] for which in runners}
    for _ in range(a.evals):
        for which, fn in runners.items():
            times[which].append(run(fn))
    med = {which: statistics.median(t) for which, t in times.items()}
    emit(f"# C3 full size, B = {B}: robust(x, steps=4) against complete(x, ones, steps=4) -- each 5 tangent sweeps + 5 primal decodes + "
         f"1 encode, 5 weighted steps and 5 launches of robust_weights / weighted_residual_sqnorm --, host clock, median of {a.evals} "
         f"alternated calls each")
    for which in runners:
        emit(f"{which:26s} {med[which]:8.2f} ms  ({sorted(round(t, 2) for t in times[which])})")
    emit(f"robust / complete = {med['robust(steps=4)'] / med['complete(steps=4)']:.3f}")
    with E.timing(lambda name: True) as timer:
        proj.robust(xc)
    by = timer.by_name()
    total = sum(v[1] for v in by.values())
    emit(f"# kernel families of one robust call, ms by the engine's timer (sum {total:.2f}): robust_weights "
         f"{by['robust_weights'][1]:.3f} in {by['robust_weights'][0]} launches, weighted_gauss_newton_step "
         f"{by['weighted_gauss_newton_step'][1]:.3f} in {by['weighted_gauss_newton_step'][0]}, the rest (sweeps, decodes, encode) "
         f"{total - by['robust_weights'][1] - by['weighted_gauss_newton_step'][1]:.2f}")
    out, ref = last["robust"], last["complete"]
    emit(f"# those calls: robust info != 0: {int((out['info'] != 0).sum())}, accepted {float(out['accepted'].float().mean()):.2f} mean "
         f"(complete {float(ref['accepted'].float().mean()):.2f}), effective / D in [{float(out['effective'].min()) / 784:.3f}, "
         f"{float(out['effective'].max()) / 784:.3f}], scale in [{float(out['scale'].min()):.3e}, {float(out['scale'].max()):.3e}]")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
