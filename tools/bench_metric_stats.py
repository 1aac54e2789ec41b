#!/usr/bin/env python3
"""Cost of the metric statistics: the accumulate launches beside the Gram + Cholesky launches at the head's shapes,
and one ``MetricStatistics.update`` against one ``elbo`` on the full-size C3 model.

    python tools/bench_metric_stats.py [--reps 30] [--evals 6] [--out profiles/metric_stats.txt]

Kernels: seeded inputs at C3 (B = 512, d = 64, D = 784), C5 (B = 256, d = 128, D = 3072) and (B = 8, d = 512, D = 3072); HIP events
around ``engine.metric_stats_accumulate`` (partial + fold launches, with sample_macs) and around ``engine.gram_cholesky(T, d, 1)`` on a
random panel-layout Jacobian stack, after warm-up, median of --reps.  End to end: full-size C3 (recipe seed 0), B = 512 seeded
inputs, ``update(x)`` (latent coordinates) and ``elbo(add_offdiagonal_metric_reg=True)`` on the dequantisation-free model, host
clock around each call ending in a synchronise, alternated, medians of --evals each.  Fails without a GPU."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metric_stats.txt"))
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict

    assert torch.cuda.is_available(), "bench_metric_stats needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(0)
    emit(f"# accumulate (cmf_metric_stats_accumulate: partial + fold, chunk {E.METRIC_STATS_CHUNK}, with sample_macs) beside the Gram + "
         f"Cholesky launches (cmf_gram_cholesky, one attempt), HIP events, median of {a.reps}")
    for label, B, d, D in (("C3", 512, 64, 784), ("C5", 256, 128, 3072), ("d512", 8, 512, 3072)):
        nc = E.ceil16(d)
        T = E.Tangent(B, D, nc, "panel", "cuda", data=(torch.randn(B * D * nc, generator=gen) / D ** 0.5).cuda())
        jtj = E.gram_cholesky(T, d, 1).jtj
        state = torch.zeros(E.metric_stats_state_size(d), dtype=torch.float64, device="cuda")
        ws = torch.empty(E.metric_stats_workspace_size(B, d), dtype=torch.float64, device="cuda")
        macs = torch.empty(B, dtype=torch.float32, device="cuda")
        acc = event_ms(lambda: E.metric_stats_accumulate(jtj, state, workspace=ws, sample_macs=macs), a.reps)
        gram = event_ms(lambda: E.gram_cholesky(T, d, 1), a.reps)
        m_acc, m_gram = statistics.median(acc), statistics.median(gram)
        nbytes = 4.0 * B * d * d
        emit(f"{label:5s} B = {B:3d} d = {d:3d}: accumulate {m_acc * 1e3:8.1f} us (min {min(acc) * 1e3:.1f}; {nbytes / 1e6:.1f} MB of jtj "
             f"-> {nbytes / m_acc / 1e9:.3f} TB/s), gram_cholesky {m_gram * 1e3:9.1f} us (min {min(gram) * 1e3:.1f}), "
             f"accumulate / gram_cholesky = {m_acc / m_gram:.3f}")
        del T

    cfg = cmf_amd.get_config("mnist", latent_dimension=64, log_jacobian_method="cholesky")
    B = a.batch
    x = torch.randint(0, 256, (B, 1, 28, 28), generator=gen).float() + torch.rand(B, 1, 28, 28, generator=gen)
    dens = cmf_amd.get_density(cmf_amd.get_schema(cfg), x[:2])
    dens.load_state_dict(fill_state_dict(dens.state_dict(), seed=0))
    dens = dens.cuda().eval()
    model = dens.module.density                     # past the dequantisation wrapper: both calls see the same input
    stats = cmf_amd.MetricStatistics(model)
    xc = x.cuda()

    def run(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            if which == "update":
                stats.update(xc)
            else:
                model.elbo(xc, add_offdiagonal_metric_reg=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    run("elbo"), run("update")
    times = {"elbo": [], "update": []}
    for _ in range(a.evals):
        for which in ("elbo", "update"):
            times[which].append(run(which))
    t_elbo, t_update = statistics.median(times["elbo"]), statistics.median(times["update"])
    r = stats.result()
    emit(f"# C3 full size, B = {B}: one update (latent coordinates) against one elbo(add_offdiagonal_metric_reg=True), host clock, "
         f"median of {a.evals} alternated calls each")
    emit(f"elbo    {t_elbo:8.2f} ms  ({sorted(round(t, 2) for t in times['elbo'])})")
    emit(f"update  {t_update:8.2f} ms  ({sorted(round(t, 2) for t in times['update'])})")
    emit(f"update / elbo = {t_update / t_elbo:.3f}")
    emit(f"# statistics of the {r['count']} accumulated samples ({r['skipped']} skipped): macs {r['macs']:.4f}, macs_offdiag "
         f"{r['macs_offdiag']:.4f}, least / most prominent dimension {int(r['ranking'][0])} / {int(r['ranking'][-1])}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
