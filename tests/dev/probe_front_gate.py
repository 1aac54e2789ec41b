"""Gate of the probe front (csrc/probe_front.hip): today's block-0 conv1 launch (64 -> 64 on every Jacobian column, float relu'
factor, store filter) against {the same launch on the probe columns + the apply kernel}, at the headline's two checkerboard shapes
(B = 512, randn activations = ~50 % live rows): 28 x 28 with cin = 1 at nc = 64, 14 x 14 with cin = 2 at nc = 64 and 48.

    python tests/dev/probe_front_gate.py [--lib PATH] [--no-probe] [--batch 512] [--iters 10]

``--lib`` loads another build of libcmf_amd.so (the parent's, with ``--no-probe``: it has no apply kernel); run the parent's and
the new library alternately, twice each, in one session.  conv0 on the probe columns is cached per parameter version and is not
part of the timed calls; ``probe_uncached_ms`` times the front with that cache emptied before every call.  Prints one JSON line:
milliseconds per call (median over ``--iters``)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch

SHAPES = [(28, 28, 1, 64), (14, 14, 2, 64), (14, 14, 2, 48)]          # H, W, cin, nc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--no-probe", action="store_true")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from cmf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    if args.no_probe:
        _lib.SIGNATURES.pop("cmf_probe_apply", None)                  # the parent's library does not export it
    from cmf_amd import engine as E
    B, C = args.batch, 64
    out = dict(tag=args.tag, lib=os.path.basename(os.path.dirname(_lib.LIB_PATH)), batch=B)
    for H, W, cin, nc in SHAPES:
        HW = H * W
        gen = torch.Generator(device="cuda").manual_seed(H + cin + nc)
        rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
        ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        mask = np.broadcast_to(((ii + jj) % 2 == 1).astype(np.float32), (cin, H, W)).copy()
        host = E.probe_plan(mask)
        plan = {"ns": host["ns"], "cls": torch.from_numpy(host["cls"]).cuda(), "probes": torch.from_numpy(host["probes"]).reshape(-1).cuda()}
        view = E.NetView(E.Geometry((cin, H, W)), cin, mask=torch.from_numpy(mask).cuda(), probe=plan)
        T = E.Tangent(B, cin * HW, nc, "panel", "cuda", data=rn(B * cin * HW * nc))
        conv0 = torch.nn.Conv2d(cin, C, 3, padding=1, bias=False).cuda()
        conv1 = torch.nn.Conv2d(C, C, 3, padding=1, bias=False).cuda()
        a0, c1 = rn(B, C, H, W), rn(B, C, H, W)
        ym = E.relu_bits(c1)
        factor = dict(fmode=E.F_RELU, f=a0, f_np=C * HW, f_ci=HW, f_px=1, f_group=1)
        hd, hsl = (C * HW * nc, 16, C * nc), C * 16
        h = torch.empty(B * HW * C * nc, device="cuda")
        E.conv_tangent(T.data, 0, T.t_b, HW * nc, nc, conv0.weight, 9, h, *hd, B, cin, C, H, W, nc, fmode=E.F_RAW, f=view.mask, f_np=0, f_ci=HW,
                       f_px=1, y_sl=hsl)
        u_old, u_new = torch.zeros(B * HW * C * nc, device="cuda"), torch.zeros(B * HW * C * nc, device="cuda")
        scratch = torch.empty(B * HW * C * 16 * plan["ns"], device="cuda")

        def today():
            E.conv_tangent(h, 0, *hd, conv1.weight, 9, u_old, *hd, B, C, C, H, W, nc, x_sl=hsl, y_sl=hsl, ymask=ym, precision="bf16x3", **factor)

        def probe():
            with E.scope(E.KernelConfig(tangent="bf16x3")):
                E.probe_front(conv0, conv1, T, view, plan, factor, ym, scratch, u_new, H, W)

        def probe_uncached():
            E.DERIVED._store.clear()
            probe()

        def ms(fn):
            for _ in range(3):
                fn()
            ts = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            ts.sort()
            return round(ts[len(ts) // 2], 4)

        key = f"{H}x{W}_cin{cin}_nc{nc}"
        out[key] = dict(today_ms=ms(today))
        if not args.no_probe:
            out[key]["probe_ms"] = ms(probe)
            out[key]["probe_uncached_ms"] = ms(probe_uncached)
            live = (c1 > 0).reshape(B, C, HW).permute(0, 2, 1).reshape(B, HW, 1, C, 1)
            a, b = (t.view(B, HW, nc // 16, C, 16) * live for t in (u_new, u_old))
            out[key]["max_abs_diff_over_max"] = float((a - b).abs().max()) / float(b.abs().max())
        del h, u_old, u_new, scratch, T
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
