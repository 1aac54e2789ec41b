#!/usr/bin/env python3
"""Cost of the operator kernel of the recovery of linear inverse problems: the ``engine.operator_apply`` launch and
its image-only mode at the head's shapes, beside the ``engine.gram_cholesky(K, d, 1)`` attempt and the ``engine.gauss_newton_step``
that follow it on the M-row stack K, the data-space launch ``engine.operator_apply_wrapped`` next to it, and one
``ManifoldProjector.recover(steps=4)`` -- in head space and in data space -- against ``project(steps=4)`` on the full-size C3 model.

    python tools/bench_recovery.py [--reps 20] [--evals 6] [--out profiles/recovery.txt] [--launches-only]

Kernel: seeded random panel-layout Jacobian stacks at C3 (B = 512, D = 784, nc = 64) with M = 32, 196, 784 and C5 (B = 256,
D = 3072, nc = 128) with M = 256, a seeded Gaussian operator scaled by 1 / sqrt(D), random x_hat and y, damping 1e-3.  HIP events
around one launch (the output allocations are inside the bracket, served by the caching allocator after the warm-up), median of
--reps after three warm-up launches.  The byte figure is the one the engine's timer entry counts: J once per group of 256 rows
of the operator, K out, x_hat, y_hat and the operator once -- the operator's re-reads by every workgroup are L2's and are not
counted, so bytes / time understates the traffic of the launch where the operator is large.  What to read off: how far the launch
is from one HBM pass over J.  The wrapped launch runs on the same inputs under mnist's wrapper (scalar-mult 0.00390624, scalar-add
1e-6, logit) into a ``scale`` buffer it is given; the plain launch is the baseline.  Its ``scale`` kernel has no entry point of its
own: its time comes from a kernel trace of ``--launches-only`` (the file's last lines say how).  End to end: full-size C3 (recipe
seed 0), B = 512 seeded inputs past the dequantisation wrapper, M = 196, host clock around work that ends in a synchronise,
alternated, medians of --evals; the data-space problem measures the pixel values with the same operator.  Fails without a GPU."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

#: mnist's fused pre-head wrapper (wa, wc, logit)
WRAPPER = (0.00390624, 1e-6, True)


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--evals", type=int, default=6)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recovery.txt"))
    ap.add_argument("--launches-only", action="store_true", help="the launch table alone, nothing written: what a kernel trace runs")
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict

    assert torch.cuda.is_available(), "bench_recovery needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit(f"# operator launch (cmf_operator_apply: K = a J by fp32 MFMA and y_hat = a x_hat in float64, one workgroup per (sample, 64 "
         f"columns, <= 256 rows of a)) and its image-only mode, beside gram_cholesky(K, d, 1) and gauss_newton_step on the M-row stack; "
         f"HIP events, median of {a.reps}")
    for label, B, d, D, Ms in (("C3", 512, 64, 784, (32, 196, 784)), ("C5", 256, 128, 3072, (256,))):
        nc = E.ceil16(d)
        T = E.Tangent(B, D, nc, "panel", "cuda", data=(torch.randn(B * D * nc, generator=gen) / D ** 0.5).cuda())
        xhat = torch.randn(B, D, generator=gen).cuda()
        lam = torch.full((B,), 1e-3, dtype=torch.float64, device="cuda")
        mb_j = 4.0 * B * D * nc / 1e6
        for M in Ms:
            op = (torch.randn(M, D, generator=gen) / D ** 0.5).cuda()
            y = torch.randn(B, M, generator=gen).cuda()
            with E.timing(lambda name: name == "operator_apply") as timer:
                K, yhat = E.operator_apply(T, op, xhat)
            counted = timer.by_name()["operator_apply"][3]
            jtj = E.gram_cholesky(K, d, 1).jtj
            full = event_ms(lambda: E.operator_apply(T, op, xhat), a.reps)
            image = event_ms(lambda: E.operator_image(op, xhat), a.reps)
            gram = event_ms(lambda: E.gram_cholesky(K, d, 1), a.reps)
            step = event_ms(lambda: E.gauss_newton_step(K, jtj, y, yhat, lam), a.reps)
            info = E.gauss_newton_step(K, jtj, y, yhat, lam).info.cpu()
            m_full, m_image, m_gram, m_step = (statistics.median(v) for v in (full, image, gram, step))
            scale = torch.empty(B, D, device="cuda")
            with E.timing(lambda name: name == "operator_apply_wrapped") as timer:
                E.operator_apply_wrapped(T, op, xhat, WRAPPER, scale)
            counted_w = timer.by_name()["operator_apply_wrapped"][3]
            wfull = event_ms(lambda: E.operator_apply_wrapped(T, op, xhat, WRAPPER, scale), a.reps)
            wimage = event_ms(lambda: E.operator_image_wrapped(op, xhat, WRAPPER), a.reps)
            m_wfull, m_wimage = statistics.median(wfull), statistics.median(wimage)
            emit(f"{label:3s} B = {B:3d} D = {D:4d} nc = {nc:3d} M = {M:3d}: operator_apply {m_full * 1e3:8.1f} us (min {min(full) * 1e3:.1f}; "
                 f"{counted / 1e6:.0f} MB counted = {counted / m_full / 1e6:.0f} GB/s; one pass over the {mb_j:.0f} MB of J alone would "
                 f"be {mb_j / m_full:.0f} GB/s, J is read {-(-M // 256)} x); image-only {m_image * 1e3:6.1f} us; gram_cholesky(K) "
                 f"{m_gram * 1e3:7.1f} us; gauss_newton_step(K) {m_step * 1e3:7.1f} us, info != 0: {int((info != 0).sum())}")
            emit(f"{'':37s}operator_apply_wrapped {m_wfull * 1e3:8.1f} us (min {min(wfull) * 1e3:.1f}; x {m_wfull / m_full:.3f} of the "
                 f"plain launch; {counted_w / 1e6:.0f} MB counted = {counted_w / m_wfull / 1e6:.0f} GB/s); image-only wrapped "
                 f"{m_wimage * 1e3:6.1f} us (x {m_wimage / m_image:.3f})")
        del T
    if a.launches_only:
        return

    cfg = cmf_amd.get_config("mnist", latent_dimension=64, log_jacobian_method="cholesky")
    B, M = a.batch, 196
    x = torch.randint(0, 256, (B, 1, 28, 28), generator=gen).float() + torch.rand(B, 1, 28, 28, generator=gen)
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), x[:2])
    dens.load_state_dict(fill_state_dict(dens.state_dict(), seed=0))
    dens = dens.cuda().eval()
    model = dens.module.density                     # past the dequantisation wrapper: both sides see the same input
    proj = cmf_amd.ManifoldProjector(model, steps=4)
    xc = x.cuda()
    with torch.no_grad():
        hx = proj.head_input(xc).flatten(1)
    D = hx.shape[1]
    op = (torch.randn(M, D, generator=gen) / D ** 0.5).cuda()
    y = (hx.double() @ op.double().t()).float().contiguous()
    y_data = (xc.flatten(1).double() @ op.double().t()).float().contiguous()       # the same operator on the pixel values
    last = {}

    def project():
        last["project"] = proj.project(xc)

    def recover():
        last["recover"] = proj.recover(y, op, x_init=xc)

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def recover_data():
        last["recover_data"] = proj.recover(y_data, op, x_init=xc, space="data")

    runners = {"recover(steps=4)": recover, "recover(data, steps=4)": recover_data, "project(steps=4)": project}
    for fn in runners.values():
        run(fn)
    times = {which: [] for which in runners}
    for _ in range(a.evals):
        for which, fn in runners.items():
            times[which].append(run(fn))
    med = {which: statistics.median(t) for which, t in times.items()}
    emit(f"# C3 full size, B = {B}, M = {M} Gaussian measurements of the head's input: one recover(y, A, x_init=x, steps=4) against one "
         f"project(x, steps=4) -- the same 5 tangent sweeps + 5 primal decodes + 1 encode, plus 5 operator launches and 5 image-only "
         f"launches --, host clock, median of {a.evals} alternated calls each")
    for which in runners:
        emit(f"{which:22s} {med[which]:8.2f} ms  ({sorted(round(t, 2) for t in times[which])})")
    emit(f"recover / project = {med['recover(steps=4)'] / med['project(steps=4)']:.3f}")
    emit(f"recover(space='data') / recover = {med['recover(data, steps=4)'] / med['recover(steps=4)']:.3f}  "
         f"(the same launches, the operator kernel's two wrapped and 5 scale launches more)")
    for which, name in (("recover", "that recovery"), ("recover_data", "the data-space recovery")):
        out = last[which]
        c, c0 = out["cost"].cpu(), out["initial_cost"].cpu()
        emit(f"# {name}: cost / initial_cost in [{float((c / c0).min()):.3e}, {float((c / c0).max()):.3e}], accepted "
             f"{int(out['accepted'].min())} .. {int(out['accepted'].max())}, info != 0: {int((out['info'] != 0).sum())}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
