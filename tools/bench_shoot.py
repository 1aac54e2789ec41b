#!/usr/bin/env python3
"""Cost of geodesic shooting: one evaluation of Hamilton's right-hand side on the full-size C3 model at 32 samples
(d = 64, D = 784), split into its parts, and one ``ManifoldGeodesic.shoot_latents`` of a few steps.

    python tools/bench_shoot.py [--reps 20] [--steps 4] [--out profiles/shoot.txt]

Full-size C3 (recipe seed 0) past the dequantisation wrapper, seeded inputs, the encoder's latents, a seeded velocity and its
momentum.  Each part is bracketed by HIP events in the order the evaluation runs them, on the state the part before it left: the
primal decode that keeps state, the unsaved d-column sweep with the Gram launch, ``cmf_metric_solve``, the saved 16-column sweep over
the velocity, the backward (with the copy of the stack it consumes); median of --reps.  The whole evaluation and the whole shoot
are timed the same way.  Fails without a GPU."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shoot.txt"))
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict

    assert torch.cuda.is_available(), "bench_shoot needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    med = statistics.median
    B = a.batch
    cfg = cmf_amd.get_config("mnist", latent_dimension=64, log_jacobian_method="cholesky")
    x = torch.randint(0, 256, (B, 1, 28, 28), generator=gen).float() + torch.rand(B, 1, 28, 28, generator=gen)
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), x[:2])
    dens.load_state_dict(fill_state_dict(dens.state_dict(), seed=0))
    dens = dens.cuda().eval()
    model = dens.module.density                     # past the dequantisation wrapper
    geo = cmf_amd.ManifoldGeodesic(model, shoot_steps=a.steps)
    head, prog = geo.head, geo.head.program
    d = prog.d
    with torch.no_grad(), E.scope(head.kernels):
        z = geo.projector.head_input_and_latent(x.cuda())[1]
        v0 = torch.randn(B, d, generator=gen, dtype=torch.float64).cuda() * 0.1
        p = E.metric_solve(geo._metric(z)[2], v0, apply=True).out64
    grads = E.GradPool([q for q in head.parameters() if q.requires_grad], "cuda")

    parts = ["primal decode (state kept)", "d-column sweep + gram", "cmf_metric_solve", "16-column saved sweep", "backward"]
    times = {k: [] for k in parts + ["evaluation"]}

    def split_evaluation(record):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(parts) + 1)]
        with torch.no_grad(), E.scope(head.kernels):
            ev[0].record()
            x_hat, _, pctx = prog.decode_train(z, tangents=False, nc_hint=16)
            ev[1].record()
            T, _ = prog.decode_tangents_from_ctx(pctx)
            jtj = E.gram_cholesky(T, d, 1).jtj
            del T
            ev[2].record()
            r = E.metric_solve(jtj, p)
            ev[3].record()
            TV, ctx = prog.decode_tangents_from_ctx(pctx, eps=r.out32[:, :, None], nc=16, save=True)
            ev[4].record()
            Ct = E.Tangent(TV.B, TV.N, TV.nc, TV.layout, TV.data.device, data=TV.data.clone(), compact=TV.compact)
            prog.decode_backward(ctx, Ct, torch.zeros_like(x_hat), grads)
            ev[5].record()
        torch.cuda.synchronize()
        if record:
            for k, e0, e1 in zip(parts, ev[:-1], ev[1:]):
                times[k].append(e0.elapsed_time(e1))
        return r.info

    def whole(fn, key, record):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if record:
            times.setdefault(key, []).append(e0.elapsed_time(e1))
        return out

    for i in range(3 + a.reps):
        info = split_evaluation(i >= 3)
        whole(lambda: geo.shoot_evaluate(z, p, grads), "evaluation", i >= 3)
    emit(f"# one evaluation of the right-hand side (ManifoldGeodesic.shoot_evaluate) on full-size C3, {B} samples, d = {d}, D = 784: "
         f"HIP events around each part, median of {a.reps} (min); info != 0: {int((info != 0).sum())}")
    total = sum(med(times[k]) for k in parts)
    for k in parts:
        emit(f"{k:28s} {med(times[k]):9.3f} ms (min {min(times[k]):.3f})  {100 * med(times[k]) / total:5.1f} % of the parts")
    emit(f"{'sum of the parts':28s} {total:9.3f} ms; the evaluation in one bracket {med(times['evaluation']):.3f} ms "
         f"(min {min(times['evaluation']):.3f})")

    key = f"shoot_latents(steps={a.steps})"
    for i in range(1 + max(3, a.reps // 4)):
        out = whole(lambda: geo.shoot_latents(z, v0), key, i >= 1)
    s2 = out["speed2"].cpu()
    emit(f"# {key}: {4 * a.steps + 1} evaluations ({4 * a.steps} with the backward), the momentum of v0 and the map back to data space")
    emit(f"{key:28s} {med(times[key]):9.3f} ms (min {min(times[key]):.3f}) = {med(times[key]) / med(times['evaluation']):.2f} evaluations; "
         f"steps_taken {int(out['steps_taken'].min())} .. {int(out['steps_taken'].max())}, info != 0: {int((out['info'] != 0).sum())}, "
         f"max |speed2 / speed2_0 - 1| = {float((s2 / s2[:, :1] - 1).abs().max()):.3e} (ResNet couplers: jumps at ReLU boundaries)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
