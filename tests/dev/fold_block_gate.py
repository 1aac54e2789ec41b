"""Gate of the folded block (csrc/conv_block_head.hip): today's {last block's conv1 with its store filter + folded head} against the
one launch that takes conv1 in as well, at the headline's checkerboard shapes (B = 512, random relu' bits = ~50 % live rows).

    python tests/dev/fold_block_gate.py [--lib PATH] [--parent] [--batch 512] [--iters 10] [--shape 28,28,2,64] [--tag T]

``--lib`` loads another build of libcmf_amd.so (the parent's, with ``--parent``: it has neither the new kernel nor the pack entry,
and only today's pair is timed); run the parent's and the new library alternately, twice each, in one session.  The W1 pack is
cached per parameter version and is not part of the timed calls.  ``--shape H,W,cout,nc`` may be given several times.  Prints one
JSON line per shape: milliseconds per call (median over ``--iters``, HIP events)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shape", action="append")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from cmf_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    if args.parent:
        _lib.SIGNATURES.pop("cmf_pack_block_weight", None)             # the parent's library does not export it
    from cmf_amd import engine as E
    shapes = [tuple(int(v) for v in s.split(",")) for s in (args.shape or ["28,28,2,64", "14,14,4,64", "14,14,4,48"])]
    B, C = args.batch, 64
    for H, W, cout, nc in shapes:
        HW = H * W
        out = dict(tag=args.tag, lib=os.path.basename(os.path.dirname(_lib.LIB_PATH)), batch=B, H=H, W=W, cout=cout, nc=nc)
        gen = torch.Generator(device="cuda").manual_seed(28)
        rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
        conv1 = torch.nn.Conv2d(C, C, 3, padding=1, bias=False).cuda()
        conv2 = torch.nn.Conv2d(C, C, 3, padding=1, bias=False).cuda()
        convf = torch.nn.Conv2d(C, cout, 1, bias=False).cuda()
        ma, m1, aK = E.relu_bits(rn(B, C, H, W)), E.relu_bits(rn(B, C, H, W)), rn(B, C, H, W)
        hd, hsl = (C * HW * nc, 16, C * nc), C * 16
        h = rn(B * HW * C * nc)
        u = torch.zeros(B * HW * C * nc, device="cuda")
        HWo = HW // 2
        y_old, y_new = torch.zeros(B * cout * HWo * nc, device="cuda"), torch.zeros(B * cout * HWo * nc, device="cuda")
        ys = (cout * HWo * nc, HWo * nc, nc)

        def conv1_filtered():
            E.conv_tangent(h, 0, *hd, conv1.weight, 9, u, *hd, B, C, C, H, W, nc, x_sl=hsl, y_sl=hsl, precision="bf16x3", fmode=E.F_RELU_BITS,
                           f=ma.data, f_np=ma.np_bytes, ymask=m1)

        def folded_head():
            E.conv_tangent(u, 0, *hd, conv2.weight, 9, y_old, *ys, B, C, C, H, W, nc, res_t=h, res_np=hd[0], x_sl=hsl, live=1,
                           precision="bf16x3", fmode=E.F_RELU_BITS, f=m1.data, f_np=m1.np_bytes, head=dict(weight=convf.weight, act=aK))

        def folded_block():
            E.conv_tangent(h, 0, *hd, conv2.weight, 9, y_new, *ys, B, C, C, H, W, nc, x_sl=hsl, live=1, precision="bf16x3",
                           fmode=E.F_RELU_BITS, f=ma.data, f_np=ma.np_bytes,
                           head=dict(weight=convf.weight, act=aK, conv1=dict(weight=conv1.weight, mask=m1)))

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

        out["conv1_ms"], out["head_ms"] = ms(conv1_filtered), ms(folded_head)
        out["today_ms"] = round(out["conv1_ms"] + out["head_ms"], 4)
        if not args.parent:
            out["block_ms"] = ms(folded_block)
            out["max_abs_diff_over_max"] = float((y_new - y_old).abs().max()) / float(y_old.abs().max())
        print(json.dumps(out), flush=True)
        del h, u, y_old, y_new
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
