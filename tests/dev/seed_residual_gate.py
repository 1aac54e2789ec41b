"""Gate of the seeded residual (MODE 8 of csrc/conv_tangent_bf16x3.hip): today's {thin conv0 on every Jacobian column + block 0's
conv2 with h0 as its residual} against {seed panel + seeded conv2}, at the headline's 28 x 28 checkerboard shape (B = 512, nc = 64,
cin = 1, random relu' bits = ~50 % live rows).

    python tests/dev/seed_residual_gate.py [--lib PATH] [--no-seed] [--batch 512] [--iters 10] [--dump PATH]

``--lib`` loads another build of libcmf_amd.so (the parent's, with ``--no-seed``: it has neither the seeded mode nor the panel
kernel); run the parent's and the new library alternately, twice each, in one session.  The seed pack of conv0's weight is cached per
parameter version and is not part of the timed calls.  ``--dump PATH`` also writes the plain residual launch of
tests/test_gpu_seed_residual.py (``plain_launch``) as a .npy -- run once with the parent's library, the file is that test's golden.
Prints one JSON line: milliseconds per call (median over ``--iters``)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--no-seed", action="store_true")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tag", default="")
    ap.add_argument("--dump")
    args = ap.parse_args()
    from cmf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    if args.no_seed:
        for name in ("cmf_seed_panel", "cmf_pack_seed_weight"):    # the parent's library does not export them
            _lib.SIGNATURES.pop(name, None)
    from cmf_amd import engine as E
    if args.dump:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_gpu_seed_residual as TS
        np.save(args.dump, TS.plain_launch(E, TS.plain_launch_inputs()).numpy())
    B, C, H, W, nc = args.batch, 64, 28, 28, 64
    HW = H * W
    out = dict(tag=args.tag, lib=os.path.basename(os.path.dirname(_lib.LIB_PATH)), batch=B)
    gen = torch.Generator(device="cuda").manual_seed(28)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mask = ((ii + jj) % 2 == 1).astype(np.float32)[None].copy()
    view = E.NetView(E.Geometry((1, H, W)), 1, mask=torch.from_numpy(mask).cuda())
    T = E.Tangent(B, HW, nc, "panel", "cuda", data=rn(B * HW * nc))
    conv0 = torch.nn.Conv2d(1, C, 3, padding=1, bias=False).cuda()
    conv2 = torch.nn.Conv2d(C, C, 3, padding=1, bias=False).cuda()
    bits = E.relu_bits(rn(B, C, H, W))
    factor = dict(fmode=E.F_RELU_BITS, f=bits.data, f_np=bits.np_bytes)
    hd, hsl = (C * HW * nc, 16, C * nc), C * 16
    u = rn(B * HW * C * nc)
    h = torch.empty(B * HW * C * nc, device="cuda")
    y_old, y_new = torch.zeros(B * HW * C * nc, device="cuda"), torch.zeros(B * HW * C * nc, device="cuda")
    sd = {}

    def thin():
        E.conv_tangent(T.data, 0, T.t_b, HW * nc, nc, conv0.weight, 9, h, *hd, B, 1, C, H, W, nc, fmode=E.F_RAW, f=view.mask, f_np=0, f_ci=HW,
                       f_px=1, y_sl=hsl)

    def conv2_residual():
        E.conv_tangent(u, 0, *hd, conv2.weight, 9, y_old, *hd, B, C, C, H, W, nc, res_t=h, x_sl=hsl, y_sl=hsl, precision="bf16x3", **factor)

    def conv2_plain():
        E.conv_tangent(u, 0, *hd, conv2.weight, 9, y_old, *hd, B, C, C, H, W, nc, x_sl=hsl, y_sl=hsl, precision="bf16x3", **factor)

    def panel():
        sd.update(E.seed_panel(T, view, H, W))

    def conv2_seeded():
        E.conv_tangent(u, 0, *hd, conv2.weight, 9, y_new, *hd, B, C, C, H, W, nc, x_sl=hsl, y_sl=hsl, precision="bf16x3",
                       seed=dict(sd, pack=E._seed_pack(conv0, "cuda")), **factor)

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

    out["thin_ms"], out["conv2_plain_ms"], out["conv2_residual_ms"] = ms(thin), ms(conv2_plain), ms(conv2_residual)
    out["today_ms"] = round(out["thin_ms"] + out["conv2_residual_ms"], 4)
    if not args.no_seed:
        out["panel_ms"], out["conv2_seeded_ms"] = ms(panel), ms(conv2_seeded)
        out["seeded_ms"] = round(out["panel_ms"] + out["conv2_seeded_ms"], 4)
        conv2_residual()
        out["max_abs_diff_over_max"] = float((y_new - y_old).abs().max()) / float(y_old.abs().max())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
