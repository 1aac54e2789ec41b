#!/usr/bin/env python3
"""Cost of the curvature reduction: the per-sample second-form launch (``cmf_second_form``) beside one Gram + Cholesky
attempt at the head's shapes.

    python tools/bench_curvature.py [--reps 20] [--out profiles/curvature.txt]

Kernel: seeded random panel-layout stacks at (B, d, m, D) = (256, 64, 4, 784) (C3) and (16, 128, 4, 3072) (C5): a centre stack of d
columns, its Gram matrices from ``engine.gram_cholesky(T, d, 1)``, and a 16-column shifted stack of 2 m B samples whose first m columns
are the centre columns along a seeded unit frame plus a seeded second-derivative term of size h = 2^-7.  ``engine.timing`` brackets
every launch with HIP events; the median of --reps launches after a warm-up of three, with the wrapper's own FLOP and byte counts.
Fails without a GPU."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_ms(name, fn, reps):
    """(per-launch ms of the ``name`` entries of ``engine.timing`` over ``reps`` calls of ``fn`` after three warm-up calls, flops, bytes)"""
    from cmf_amd import engine as E
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with E.timing(lambda n: n == name) as t:
        for _ in range(reps):
            fn()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for _, _, _, e0, e1 in t.records], t.records[0][1], t.records[0][2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curvature.txt"))
    a = ap.parse_args()
    from cmf_amd import engine as E

    assert torch.cuda.is_available(), "bench_curvature needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    med = statistics.median
    h = 2.0 ** -7
    emit(f"# second-form launch (cmf_second_form: per sample the float64 J^T H stream over D rows, H^T H, a float64 Cholesky of G with "
         f"q = m (m + 1) / 2 right-hand sides, the Schur complement and the back substitution, one workgroup per sample) beside the Gram + "
         f"Cholesky launch (cmf_gram_cholesky, one attempt), engine.timing, median of {a.reps}")
    for label, B, d, m, D in (("C3", 256, 64, 4, 784), ("C5", 16, 128, 4, 3072)):
        nc = E.ceil16(d)
        J = torch.randn(B, D, nc, generator=gen) / D ** 0.5
        frame = torch.randn(B, m, d, dtype=torch.float64, generator=gen)
        frame /= frame.norm(dim=2, keepdim=True)
        centre = torch.einsum("brj,bcj->brc", J[:, :, :d].double(), frame)                       # (B, D, m)
        second = torch.randn(B, m, 2, D, m, dtype=torch.float64, generator=gen) / D ** 0.5
        sign = torch.tensor([1.0, -1.0], dtype=torch.float64)[None, None, :, None, None]
        S = torch.zeros(B, m, 2, D, 16)
        S[..., :m] = (centre[:, None, None] + h * sign * second).float()
        T = E.Tangent(B, D, nc, "panel", "cuda", data=J.reshape(-1).cuda())
        St = E.Tangent(B * m * 2, D, 16, "panel", "cuda", data=S.reshape(-1).cuda())
        jtj = E.gram_cholesky(T, d, 1).jtj
        fr, st = frame.cuda(), torch.full((B,), h, dtype=torch.float64, device="cuda")
        gram = timed_ms("gram_cholesky", lambda: E.gram_cholesky(T, d, 1), a.reps)[0]
        sf, flops, nbytes = timed_ms("second_form", lambda: E.second_form(T, jtj, St, fr, st), a.reps)
        r = E.second_form(T, jtj, St, fr, st)
        emit(f"{label:3s} B = {B:3d}, d = {d:3d}, m = {m}, D = {D:4d}: second_form {med(sf) * 1e3:9.1f} us (min {min(sf) * 1e3:.1f}), "
             f"{flops / med(sf) * 1e-6:7.1f} GFLOP/s float64, {nbytes / med(sf) * 1e-6:7.1f} GB/s, info != 0: {int((r.info != 0).sum())}, "
             f"cancellation min {float((r.stats[:, 3] / r.stats[:, 2]).min()):.2e}; gram_cholesky {med(gram) * 1e3:7.1f} us; "
             f"second_form / gram_cholesky = {med(sf) / med(gram):.2f}")
        del T, St

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
