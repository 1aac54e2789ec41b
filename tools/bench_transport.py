#!/usr/bin/env python3
"""Cost of parallel transport: the per-curve chain launch (``cmf_transport_chain``) beside the cross-Gram launch over
the padded stack and one Gram + Cholesky attempt at the head's shapes, and what ``ManifoldGeodesic.transport`` reaches on the
fixtures.

    python tools/bench_transport.py [--reps 20] [--out profiles/transport.txt]

Kernel: seeded random panel-layout Jacobian stacks at 32 curves x 16 points with d = 64, D = 784 (C3) and 16 x 16 with d = 128,
D = 3072 (C5); every point is the first point plus a small seeded step per point, so that neighbouring tangent planes differ by
moderate angles; the stack is padded with a copy of its first and of its last sample as ``transport_latents`` does, its Gram
matrices come from ``engine.gram_cholesky(T, d, 1)`` and its cross blocks from ``engine.cross_gram(T, d, B P + 2)``; m = 1 and 16
seeded vectors.  HIP events around one launch (the output allocations are inside the bracket, served by the caching allocator after
the warm-up), median of --reps.  Fixtures: the curves of tests/test_gpu_transport.py, 9 points, 10 steps.  Fails without a GPU."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transport.txt"))
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E

    assert torch.cuda.is_available(), "bench_transport needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    med = statistics.median
    emit(f"# transport chain launch (cmf_transport_chain: per segment a float64 LU with partial pivoting and a float64 Cholesky with m "
         f"right-hand sides each, one workgroup per curve) beside the cross-Gram launch over the padded stack (cmf_cross_gram) and the "
         f"Gram + Cholesky launch (cmf_gram_cholesky, one attempt), HIP events, median of {a.reps}")
    for label, curves, P, d, D in (("C3", 32, 16, 64, 784), ("C5", 16, 16, 128, 3072)):
        B, nc = curves * P, E.ceil16(d)
        base = torch.randn(curves, 1, D, nc, generator=gen) / D ** 0.5
        walk = torch.cumsum(0.05 * torch.randn(curves, P, D, nc, generator=gen) / D ** 0.5, 1)
        J = (base + walk).reshape(B, D, nc)
        J = torch.cat([J[:1], J, J[-1:]])
        T = E.Tangent(B + 2, D, nc, "panel", "cuda", data=J.reshape(-1).cuda())
        jtj = E.gram_cholesky(T, d, 1).jtj[1:-1]
        cross = E.cross_gram(T, d, B + 2)[0]
        gram = event_ms(lambda: E.gram_cholesky(T, d, 1), a.reps)
        cr = event_ms(lambda: E.cross_gram(T, d, B + 2), a.reps)
        for m in (1, 16):
            w0 = torch.randn(curves, m, d, dtype=torch.float64, generator=gen).cuda()
            ch = event_ms(lambda: E.transport_chain(jtj, cross, w0, P), a.reps)
            r = E.transport_chain(jtj, cross, w0, P)
            drift = float((r.norm2 / r.norm2[:, :1] - 1.0).abs().max())
            gap = float(((r.fwd - r.bwd).abs().amax((1, 2, 3)) / r.out.abs().amax((1, 2, 3))).max())
            emit(f"{label:3s} {curves} curves x {P} points, d = {d:3d} D = {D:4d}, m = {m:2d}: transport_chain {med(ch) * 1e3:9.1f} us (min "
                 f"{min(ch) * 1e3:.1f}), info != 0: {int((r.info != 0).sum())}, norm2 drift {drift:.2e}, largest forward / backward gap "
                 f"{gap:.2e}; cross_gram ({B + 1} pairs) {med(cr) * 1e3:8.1f} us (min {min(cr) * 1e3:.1f}); gram_cholesky ({B + 2} samples) "
                 f"{med(gram) * 1e3:7.1f} us; transport_chain / gram_cholesky = {med(ch) / med(gram):.2f}")
        del T

    import _transport_reference as R
    from test_gpu_metric_stats import build
    from test_gpu_shoot import product_ends
    emit("# fixtures, 9 points, 10 steps, w = the log velocity and two seeded vectors: ManifoldGeodesic.transport on the product's own "
         "connect curves (bounds of tests/test_gpu_transport.py: drift 2e-3, forth and back 3e-3)")
    for name in R.FIXTURES:
        g, meta, fd, fh, fx = build(name)
        x0, x1 = product_ends(name, fx)
        geo = cmf_amd.ManifoldGeodesic(fd, points=9, steps=10)
        w = R.start_vectors(geo.log(x0, x1)["latents"].cpu()).cuda()
        tr = geo.transport(x0, x1, w)
        back = geo.transport_latents(tr["latents"].flip(1).contiguous(), tr["transported"])
        gap = float(((tr["forward"] - tr["backward"]).abs().amax((1, 2, 3)) / tr["vectors"].abs().amax((1, 2, 3))).max())
        emit(f"{name:12s} norm2 drift {R.drift(tr):.2e}; forth and back {R.rel(back['vectors'][:, -1], w):.2e}; largest forward / backward "
             f"gap {gap:.2e}; info != 0: {int((tr['transport_info'] != 0).sum())}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
