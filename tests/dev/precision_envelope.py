#!/usr/bin/env python3
"""Precision envelope of the kernel configurations against conditioning (the precision guard's default threshold).

The full-size C3 model (MNIST, d = 64, recipe seed 0) with the ScaledTanh gain raised (``recipe.apply_gain({"weights": g})``,
the knob of the c3_mnist_full_cond fixture) until cond(J^T J) spans ~1e1 .. 1e6 and beyond; B seeded MNIST-range inputs per gain,
repeated to 16 rows on the GPU so that the primal convolutions take the grouped path the configuration governs (batches that are
not a multiple of 16 run exact fp32 primal convs whatever the configuration).  The yardstick is the in-repo oracle in float64; the
oracle in float32 (the reference's own arithmetic) is recorded beside it.  Per sample: kappa_1 of the float64 J^T J, the kernel's
value (engine.gram_condition of the default configuration's J^T J), and the relative log-det and g_ij (off-diagonal metric term)
errors of the configurations (tangent, primal) = (bf16x3, f16x3) [default], (f32, f16x3) and (f32, f32).  Then the crossover
rule of DESIGN 5: the largest measured kappa_1 below which every default-configuration sample holds 1e-4 on the log-det.

    python tests/dev/precision_envelope.py [--gains 1,2,3] [--batch 3] [--out FILE]

It lives under tests/ because it imports the oracle, which the package and tools/ never do (test_host_logic).
"""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = [("bf16x3", "f16x3"), ("f32", "f16x3"), ("f32", "f32")]


def kappa1(a):
    a = a.double()
    return float(torch.linalg.matrix_norm(a, ord=1) * torch.linalg.matrix_norm(torch.linalg.inv(a), ord=1))


def relerr(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gains", default="1.0,1.5,1.9,2.2,2.4,2.6,2.75,2.9,3.0")
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cmf_amd
    from cmf_amd import engine as E
    from cmf_amd.recipe import fill_state_dict
    from oracle import cmf_oracle as O

    assert torch.cuda.is_available(), "precision_envelope needs a GPU"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    cfg = cmf_amd.get_config("mnist", latent_dimension=64, log_jacobian_method="cholesky")
    schema = cmf_amd.get_schema(cfg)
    gen = torch.Generator().manual_seed(a.seed)
    B = a.batch
    assert 1 <= B <= 16
    x = torch.randint(0, 256, (B, 1, 28, 28), generator=gen).float() + torch.rand(B, 1, 28, 28, generator=gen)
    xg = x.repeat(-(-16 // B), 1, 1, 1)[:16].cuda()              # rows 0 .. B-1 are the samples
    ops = O.compile_schema(schema, (1, 28, 28))
    emit(f"# precision envelope: C3 full size (mnist, d = 64, recipe seed 0), B = {B} seeded inputs per gain (seed {a.seed}), "
         "16 rows on the GPU")
    emit("# kappa64 = kappa_1 of the float64 oracle's J^T J; est = engine.gram_condition of the default config's J^T J;")
    emit("# errors: |value - float64 oracle| / |float64 oracle| per sample; ld = log-det, gij = off-diagonal metric term")
    hdr = f"{'gain':>5} {'s':>2} {'kappa64':>9} {'est':>9} | {'ld oracle32':>11} {'gij oracle32':>12}"
    for t, p in CONFIGS:
        hdr += f" | {'ld ' + t + '/' + p:>15} {'gij ' + t + '/' + p:>16}"
    emit(hdr)
    rows = []
    for gain in [float(v) for v in a.gains.split(",")]:
        t0 = time.time()
        dens = cmf_amd.get_density(schema, x)
        sd = fill_state_dict(dens.state_dict(), seed=0, gain={"weights": gain})
        dens.load_state_dict(sd)
        dens = dens.cuda().eval()
        model = dens.module.density                        # no dequantisation wrapper: the noise is part of x here
        head = next(m for m in dens.modules() if type(m).__name__ == "NonSquareHeadDensity")
        head.precision_guard = cmf_amd.PrecisionGuard(math.inf)    # records cond, never re-runs
        got = {}
        with torch.no_grad():
            for t, p in CONFIGS:
                head.kernels = E.KernelConfig(tangent=t, primal=p)
                model.elbo(xg, add_offdiagonal_metric_reg=True)
                g = head.last_gram
                got[(t, p)] = (g.logdet.cpu(), g.l1_off.cpu(), g.cond.cpu())
            sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
            p64 = O.elbo(sd64, ops, x.double(), noise=torch.zeros_like(x).double(), add_offdiagonal_metric_reg=True,
                         return_parts=True)["parts"]
            p32 = O.elbo(sd, ops, x, noise=torch.zeros_like(x), add_offdiagonal_metric_reg=True, return_parts=True)["parts"]
        for s in range(B):
            k64 = kappa1(p64["jtj"][s])
            ld64, l164 = float(p64["logdet"].reshape(-1)[s]), float(p64["l1"].reshape(-1)[s])
            row = {"gain": gain, "s": s, "kappa": k64, "est": float(got[CONFIGS[0]][2][s]),
                   "o32": (relerr(p32["logdet"].reshape(-1)[s], ld64), relerr(p32["l1"].reshape(-1)[s], l164))}
            line = f"{gain:5.2f} {s:2d} {k64:9.3e} {row['est']:9.3e} | {row['o32'][0]:11.2e} {row['o32'][1]:12.2e}"
            for c in CONFIGS:
                e = (relerr(got[c][0][s], ld64), relerr(got[c][1][s], l164))
                row[c] = e
                line += f" | {e[0]:15.2e} {e[1]:16.2e}"
            rows.append(row)
            emit(line)
        print(f"# gain {gain}: {time.time() - t0:.1f} s", flush=True)
    rows.sort(key=lambda r: r["kappa"])
    ok = None
    for r in rows:
        if r[CONFIGS[0]][0] > 1e-4:
            break
        ok = r["kappa"]
    first_bad = next((r for r in rows if r[CONFIGS[0]][0] > 1e-4), None)
    emit("")
    emit(f"# sweep: kappa_1 {rows[0]['kappa']:.3e} .. {rows[-1]['kappa']:.3e} over {len(rows)} samples")
    if first_bad is None:
        emit(f"# the default config holds 1e-4 on the log-det for every sample, up to kappa_1 = {rows[-1]['kappa']:.3e} (top of "
             "the sweep)")
    else:
        emit(f"# first default-config log-det error above 1e-4: kappa_1 = {first_bad['kappa']:.3e} "
             f"(error {first_bad[CONFIGS[0]][0]:.2e}, exact config {first_bad[CONFIGS[2]][0]:.2e})")
        emit(f"# crossover (largest kappa_1 below which every default-config sample holds 1e-4): "
             f"{ok if ok is not None else float('nan'):.3e}")
    f32 = [r for r in rows if r[CONFIGS[2]][0] > 1e-4]
    emit(f"# exact config (f32, f32) log-det errors above 1e-4: {len(f32)} of {len(rows)} samples"
         + (f" (smallest kappa_1 {f32[0]['kappa']:.3e})" if f32 else ""))
    fin = [abs(math.log10(max(r["est"], 1e-30) / r["kappa"])) for r in rows if math.isfinite(r["est"])]
    if fin:
        emit(f"# estimate vs kappa64 (the default config's own J^T J against the float64 one): worst factor 10^{max(fin):.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
