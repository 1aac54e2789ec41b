"""Gate of the folded head (csrc/conv_head.hip): today's {last hidden conv (checkerboard or full) + gather of the last activation +
1x1 conv} against the ONE folded launch, at the three shapes of the headline (B = 512, nc = 64, randn activations = ~50 % live rows).

    python tests/dev/fold_head_gate.py [--lib PATH] [--no-fold] [--batch 512] [--iters 10]

``--lib`` loads another build of libcmf_amd.so (the parent's, with ``--no-fold``: it has no folded launch); run the parent's and the
new library alternately, twice each, in one session.  Prints one JSON line: milliseconds per call (median over ``--iters``)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

SHAPES = [(28, 28, 1, 2), (14, 14, 1, 4), (14, 14, 0, 4)]          # H, W, live, cout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--no-fold", action="store_true")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from cmf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from cmf_amd import engine as E
    B, nc, C = args.batch, 64, 64
    out = dict(tag=args.tag, lib=os.path.basename(os.path.dirname(_lib.LIB_PATH)), batch=B, nc=nc)
    for H, W, live, cout in SHAPES:
        HW = H * W
        HWo = HW // 2 if live else HW
        gen = torch.Generator(device="cuda").manual_seed(H + live)
        rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
        u, h = rn(B, HW, nc // 16, C, 16), rn(B, HW, nc // 16, C, 16)
        c1, aK = rn(B, C, H, W), rn(B, C, H, W)
        w2, wf = torch.nn.Parameter(rn(C, C, 3, 3) / 24), torch.nn.Parameter(rn(cout, C, 1, 1) / 8)
        bits = E.relu_bits(c1)
        fk = dict(fmode=E.F_RELU_BITS, f=bits.data, f_np=bits.np_bytes)
        st, sl = (C * HW * nc, 16, C * nc), C * 16
        hK = torch.empty(B, HWo, nc // 16, C, 16, device="cuda")
        yt = torch.empty(B, cout, HWo, nc, device="cuda")
        yf = torch.empty(B, cout, HWo, nc, device="cuda")
        ii, jj = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        pix = torch.arange(HW)[((ii + jj) % 2 == live - 1).reshape(-1)] if live else torch.arange(HW)
        idx = (torch.arange(C).view(C, 1) * HW + pix.view(1, -1)).reshape(-1).to(torch.int32).cuda()

        def two():
            E.conv_tangent(u, 0, *st, w2, 9, hK, C * HWo * nc, 16, C * nc, B, C, C, H, W, nc, res_t=h, res_np=st[0], x_sl=sl, y_sl=sl,
                           live=live, precision="bf16x3", **fk)
            a = E.gather_primal(aK, idx, C * HWo) if live else aK
            E.conv_tangent(hK, 0, C * HWo * nc, 16, C * nc, wf, 1, yt, cout * HWo * nc, HWo * nc, nc, B, C, cout, H, W // 2 if live else W,
                           nc, fmode=E.F_RELU, f=a, x_sl=sl, f_np=C * HWo, f_ci=HWo, f_px=1, precision="bf16x3")

        def fold():
            E.conv_tangent(u, 0, *st, w2, 9, yf, cout * HWo * nc, HWo * nc, nc, B, C, C, H, W, nc, res_t=h, res_np=st[0], x_sl=sl,
                           live=live, precision="bf16x3", head=dict(weight=wf, act=aK), **fk)

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

        key = f"{H}x{W}_{'live' if live else 'full'}_cout{cout}"
        out[key] = dict(two_launches_ms=ms(two))
        if not args.no_fold:
            out[key]["folded_ms"] = ms(fold)
            scale = float(yt.abs().max())
            out[key]["max_abs_diff_over_max"] = float((yf - yt).abs().max()) / scale
        del u, h, hK
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
