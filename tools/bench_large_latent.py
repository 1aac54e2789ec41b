#!/usr/bin/env python3
"""Wide latents on one MI355X: evals/s and the per-stage split of the Cholesky-path log-density for C5-shaped CIFAR (D = 3072,
the C5 recipe's overrides) at d in {128, 256, 512} and MNIST at d = 256, plus one training step each; the head kernels' share of
the step is what the wide head (csrc/head_wide.hip, 128 < ceil16(d) <= 512) costs.

  python tools/bench_large_latent.py [--batch 8] [--steps 3] [--cases c5:128,c5:256,c5:512,mnist:256] [--no-train]

Prints one JSON line per case: evals/s, ms per eval, the head kernels' ms and share (eval and train step), and every timed
kernel family (the ``stages`` timer: engine.timing over all families)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                                       # noqa: E402  (make_model / synth_batch only)
from cmf_amd import engine as E                                    # noqa: E402

HEAD = ("gram_cholesky", "gram_backward", "hutch_")


def head_ms(by):
    return sum(ms for name, (n, ms, fl, b) in by.items() if name.startswith(HEAD))


def run(dataset, d, B, steps, train, dev):
    overrides = {"latent_dimension": d, "log_jacobian_method": "cholesky"}
    cfg, schema, shape, sd, density = bench.make_model(dev, dataset=dataset, overrides=overrides)
    inner = density.module.density
    x = bench.synth_batch(dataset, shape, B, 0, dev)
    kw = dict(add_reconstruction=True, add_offdiagonal_metric_reg=True)
    with torch.no_grad():
        inner.elbo(x, **kw)                                        # warm-up: packs, LDS attributes, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            inner.elbo(x, **kw)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        with E.timing(lambda name: True) as timer:
            inner.elbo(x, **kw)
        by = timer.by_name()
    out = {"dataset": dataset, "d": d, "batch": B, "evals_per_s": B / ms * 1e3, "ms_per_eval": ms,
           "head_ms": head_ms(by), "timed_ms": sum(v[1] for v in by.values()),
           "stages": {k: round(v[1], 3) for k, v in sorted(by.items(), key=lambda kv: -kv[1][1])}}
    out["head_share"] = out["head_ms"] / max(out["timed_ms"], 1e-9)
    if train:
        inner.train()

        def step():                                                # the reference's loss.backward() (trainer.py:213)
            inner.zero_grad(set_to_none=True)
            (-inner.elbo(x, **kw)["elbo"].mean()).backward()
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with E.timing(lambda name: True) as timer:
            step()
            by = timer.by_name()
        out["train_step_ms"] = (time.perf_counter() - t0) * 1e3
        out["train_head_ms"] = head_ms(by)
        out["train_timed_ms"] = sum(v[1] for v in by.values())
        out["train_head_share"] = out["train_head_ms"] / max(out["train_timed_ms"], 1e-9)
        out["train_stages"] = {k: round(v[1], 3) for k, v in sorted(by.items(), key=lambda kv: -kv[1][1]) if k.startswith(HEAD)}
        inner.eval()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--cases", default="c5:128,c5:256,c5:512,mnist:256")
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for case in args.cases.split(","):
        name, d = case.split(":")
        dataset = "cifar10" if name == "c5" else name
        print(json.dumps(run(dataset, int(d), args.batch, args.steps, not args.no_train, dev)), flush=True)


if __name__ == "__main__":
    main()
