"""Helpers shared by tests/test_gpu_persistent_items.py and tests/test_persistent_items_host.py (not collected by pytest).

The three persistent kernel families (cmf_conv_tangent_bf16x3 / _f16x3, cmf_conv_tangent_wgrad_bf16x3(_batched), the row-walking
fp32 weight gradient of conv_wgrad.hip) launch min(work, 256) workgroups and let each workgroup walk a list of work items.  This
module mirrors, from a launch's shape alone,

* how many items a launch has and how the kernels deal them to workgroups (``forward_items`` ... ``block_counts``),
* the batch size that puts a launch in the multi-item regime (``choose_np`` / ``multi_item_problems``),
* the per-element error bound of the split arithmetic (``C_BF16X3`` / ``C_F16X3`` and their derivation) with a CPU emulation of
  the three-product split (``emulate_split_conv``),
* guard-banded device buffers (``Guarded``) and the repeated-base-sample batches of the position-independence check.
"""
import math

import torch
import torch.nn.functional as F

WG_MAX = 256                      # conv_wgrad_bf16x3.hip / conv_wgrad.hip
GUARD_BYTES = 8192                # sentinel band on both sides of every output buffer (>= 4 KiB)
GUARD_FILL = 0xA5

# ---------------------------------------------------------------------------------------------------------------------------
# Error bound  |got - want| <= c * A,   A = conv2d(|F x|, |w|) (+ |res|):  c from the arithmetic, never from a kernel's output.
#
# bf16 split: x = x_hi + x_lo + dx with x_hi = bf16(x) (8 significant bits, round to nearest: |x - x_hi| <= 2^-9 |x|)
# and x_lo = bf16(x - x_hi), so |dx| <= 2^-9 * 2^-9 |x| = 2^-18 |x|; the same for w.  The kernel forms x_hi w_hi + x_hi w_lo +
# x_lo w_hi and leaves out x_lo w_lo (<= 2^-18 |x w|) and the two tails (<= 2^-18 |x w| each): at most 3 * 2^-18 < 2^-16 of |x w|
# per product, i.e. 2^-16 * A for an element if every product erred the same way.  fp32 accumulation of the 3 K products (K = 9 cin
# <= 1152) adds 2^-24 times the partial sums' magnitudes: a worst case of 3 K 2^-24 A that no data reaches, ~sqrt(3 K) 2^-24 A <=
# 2^-18.1 A if every rounding were as large as A's, far less in practice (partial sums of signed products are ~sqrt(K) times
# smaller than A).  A residual is the accumulators' initial value: every partial sum is rounded at its magnitude, which is why
# |res| is part of A.  c = 2^-16 covers the first-order term in full and the CPU emulation (tests/test_persistent_items_host.py)
# reaches 2^-18 ... 2^-19 of A: a factor of four of margin.
C_BF16X3 = 2.0 ** -16
# fp16 split: 11 + 11 significant bits with exact power-of-two operand scales: |x - x_hi| <= 2^-12 |x|, tails and the
# lo * lo product <= 2^-24 |x w| each: 3 * 2^-24 < 2^-22 per product, the size of fp32's own product rounding.  The same factor of
# four over what the emulation reaches (2^-22 of A: the fp32 accumulation is the larger part there) gives 2^-20.
C_F16X3 = 2.0 ** -20


# ---------------------------------------------------------------------------------------------------------------------------
# Launch geometry
def tile_shape(H, W):
    """Pixel tile of the split kernels: 2 x 14 when the image is a whole number of them, else 4 x 8."""
    return (2, 14) if W % 14 == 0 and H % 2 == 0 else (4, 8)


def n_tiles(H, W):
    th, tw = tile_shape(H, W)
    assert H % th == 0 and W % tw == 0, (H, W)
    return (H // th) * (W // tw)


def forward_items(H, W, nc, cout, np_, group=64):
    """Items of one cmf_conv_tangent_bf16x3 / _f16x3 launch: tile x 16-column slice x output-channel group x sample (group).
    ``group`` 32: the fp16 form's 32-channel items."""
    ncog = cout // 32 if group == 32 else -(-cout // 64)
    return n_tiles(H, W) * (nc // 16) * ncog * np_


def f16_item_group(H, W, item_channels):
    """Channel-group size the fp16 kernel runs for a request of 64 / 32: 4 x 8 tiles always take 32."""
    return 32 if tile_shape(H, W) == (4, 8) else item_channels


def wgrad_rows_split(H, nc, np_):
    """Image rows of one cmf_conv_tangent_wgrad_bf16x3 problem (a row covers a column PAIR of 16-column slices)."""
    return np_ * (nc // 32) * H


def wgrad_rows_f32(H, nc, np_):
    return np_ * (nc // 16) * H


def xcd_walk(total, G):
    """The item list of every workgroup as conv_tangent_bf16x3_kernel / conv_wgrad3x3_roles_kernel deal them: XCD k (= workgroup
    id % 8) owns a contiguous range of q or q + 1 items, its j-th workgroup takes items j, j + nbx, ...  (The weight-gradient
    kernel uses min(G, 8) ranges; below 8 workgroups both give every workgroup one item.)"""
    nx = min(G, 8)
    if nx == 0:
        return []
    q, r = divmod(total, nx)
    out = []
    for bid in range(G):
        xcd, jx = bid % nx, bid // nx
        xstart = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
        xlen = q + (1 if xcd < r else 0)
        nbx = (G - xcd + nx - 1) // nx
        out.append(list(range(xstart + jx, xstart + xlen, nbx)) if jx < xlen else [])
    return out


def xcd_counts(total, G):
    """Items per workgroup (``xcd_walk``)."""
    out = [len(w) for w in xcd_walk(total, G)]
    assert sum(out) == total, (total, G, sum(out))
    return out


def item_positions(total, G):
    """item -> (workgroup, position in that workgroup's list): where a wrong element was computed."""
    pos = {}
    for bid, items in enumerate(xcd_walk(total, G)):
        for k, w in enumerate(items):
            pos[w] = (bid, k)
    return pos


def block_counts(total, G):
    """Rows per workgroup of the fp32 row-walking weight gradient: contiguous blocks of ceil(rows / G)."""
    per = -(-total // G)
    return [max(0, min(total, (b + 1) * per) - b * per) for b in range(G)]


def multi_item_problems(total, G, per_sample=1):
    """What keeps a launch of ``total`` items on ``G`` workgroups out of the multi-item regime ([] = it is in it).
    items % 8 != 0 cannot hold for any batch size when one sample already has a multiple of 8 items (16 x 16, 32 x 32, 8 x 32
    images: 8 or 64 tiles); the condition is then void -- the XCD ranges are of equal length -- and 12 x 24 images (9 tiles of
    4 x 8) carry it for that tile form."""
    bad = []
    if total < 2 * G + 1:
        bad.append(f"items {total} < 2 G + 1 = {2 * G + 1}")
    if total % 8 == 0 and per_sample % 8 != 0:
        bad.append(f"items {total} % 8 == 0")
    if total % G == 0:
        bad.append(f"items {total} % G ({G}) == 0")
    return bad


def choose_np(per_sample, n_wg, multiple_of=1):
    """Smallest sample count (a multiple of ``multiple_of``) whose launch is in the multi-item regime; ``n_wg``: the launch's
    workgroup limit (the CU count, or 256).  Raises when there is none below 64 x the minimum."""
    lo = -(-(2 * n_wg + 1) // per_sample)
    for np_ in range(-(-lo // multiple_of) * multiple_of, 64 * lo + multiple_of, multiple_of):
        total = per_sample * np_
        if not multi_item_problems(total, min(total, n_wg), per_sample):
            return np_
    raise AssertionError(f"no batch size puts {per_sample} items per sample in the multi-item regime on {n_wg} workgroups")


def describe(total, counts):
    live = [c for c in counts if c]
    return (f"items {total}  workgroups {len(counts)}  items/workgroup {min(counts)}..{max(counts)}"
            f"  (idle workgroups {len(counts) - len(live)})")


def repeat_period(per_sample):
    """Number of distinct base samples: coprime to 8 and to the per-sample item count, so that the copies of one base sample fall
    on different XCD ranges and item positions."""
    for p in (3, 5, 7, 11, 13):
        if math.gcd(p, 8 * per_sample) == 1:
            return p
    raise AssertionError(per_sample)


def copy_plan(np_, period):
    """(base index, power-of-two exponent) of every sample of the batch: sample i is base i % period times 2^((i // period) % 4)."""
    idx = torch.arange(np_)
    return idx % period, (idx // period) % 4


# ---------------------------------------------------------------------------------------------------------------------------
# CPU emulation of the split arithmetic (tests/dev/emulate_precision.py's split(): hi / lo parts, three products, fp32 conv2d)
def split(t, dt, n):
    parts, r = [], t
    for _ in range(n):
        p = r.to(dt).to(torch.float32)
        parts.append(p)
        r = r - p
    return parts


def emulate_split_conv(x, w, dt, drop_hi_lo=False):
    """x (N, cin, H, W), w (cout, cin, 3, 3) float32 -> x_hi w_hi + x_lo w_hi + x_hi w_lo in fp32 (the last left out with
    ``drop_hi_lo``: injected defect (a) of the host test)."""
    if dt is torch.float32:
        return F.conv2d(x, w, padding=1)
    xs, ws = split(x, dt, 2), split(w, dt, 2)
    y = F.conv2d(xs[0], ws[0], padding=1) + F.conv2d(xs[1], ws[0], padding=1)
    if not drop_hi_lo:
        y = y + F.conv2d(xs[0], ws[1], padding=1)
    return y


def reference(xin, w, res=None, transpose=False):
    """float64 (want, A) of  conv2d(xin, w) [+ res]  with A = conv2d(|xin|, |w|) [+ |res|]; xin (N, cin, H, W) already factored."""
    conv = F.conv_transpose2d if transpose else F.conv2d
    xin, w = xin.double(), w.double()
    want, A = conv(xin, w, padding=1), conv(xin.abs(), w.abs(), padding=1)
    if res is not None:
        want, A = want + res.double(), A + res.double().abs()
    return want, A


def err_over_A(got, want, A):
    """max |got - want| / A over the elements (0 / 0 counts as 0: A = 0 means every product is exactly zero)."""
    err = (got.double() - want).abs()
    ratio = torch.where(A > 0, err / A.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------------------
# Guard-banded device buffers
class Guarded:
    """A flat device tensor of ``numel`` elements of ``dtype`` that is a VIEW into a larger allocation with GUARD_BYTES of
    sentinel bytes on both sides; ``check()`` asserts the bands unchanged.  ``fill``: initial value of the payload."""

    def __init__(self, numel, dtype=torch.float32, fill=float("nan"), device="cuda"):
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((nbytes + 2 * GUARD_BYTES,), GUARD_FILL, dtype=torch.uint8, device=device)
        self.t = self.raw[GUARD_BYTES:GUARD_BYTES + nbytes].view(dtype)
        assert self.t.data_ptr() % 16 == 0
        if fill is not None:
            self.t.fill_(fill)

    def check(self, what="buffer"):
        lo, hi = self.raw[:GUARD_BYTES], self.raw[-GUARD_BYTES:]
        bad_lo, bad_hi = int((lo != GUARD_FILL).sum()), int((hi != GUARD_FILL).sum())
        assert bad_lo == 0 and bad_hi == 0, f"{what}: {bad_lo} guard bytes written below, {bad_hi} above the buffer"
