"""Helpers shared by tests/test_gpu_wgrad_elements.py, tests/test_wgrad_elements_host.py and the weight-gradient cases of
tests/test_gpu_persistent_items.py (not collected by pytest).

The weight-gradient kernels -- conv_wgrad.hip: row-walking 3x3, general 1x1, the thin 3x3 / 1x1 forms, wgrad_reduce_kernel;
conv_wgrad_bf16x3.hip: single and batched -- against float64, PER ELEMENT:

    |got - want| <= c A + 2^-24 (|prev| + |want|),   want = prev + dW,   A = sum |gy| |F x|   (``reference``)

The last term is the one rounded addition of the reduced sum into ``dw``.  A == 0 marks an entry whose every product is exactly
zero (a tap wholly outside a one-row or one-column image): there the kernel must leave ``prev`` as it is, bit for bit.

c, from the arithmetic and a CPU emulation of it, never from a kernel's output:

* ``C_WGRAD_BF16X3`` = ``_persistent_items.C_BF16X3`` = 2^-16: the same three-product split per product (3 * 2^-18 < 2^-16 of every
  |gy F x|) and A already sums the products; no second constant.  The emulation reaches 2^-21.7 (14 x 14) ... 2^-17.3 (2 x 3 with
  relu: a few dozen products per entry, where single products' split errors do not average out) of A.
* ``C_WGRAD_F32``: exact products, so all of the error is fp32 rounding over R = np H W nc terms and depends on the order: per
  workgroup a chain over its K blocks (``emulate``), then wgrad_reduce_kernel's eight interleaved chains and fixed tree.  The
  rigorous (R + 8 + 1) 2^-24 A is asserted as an upper sanity bound.  MEASURED: max |emulate - want| / A of the "f32" emulation over
  every GPU case's own inputs and launch geometry (``CASES``; profiles/wgrad_elements_errors.txt has every case), worst per family:
      row-walking 3x3  2^-22.70     thin 3x3  2^-23.21 (one-row image), 2^-24.77 otherwise     thin 1x1  2^-25.26     general 1x1  2^-25.25
  The large values belong to the SMALL launches (R = 96 ... 384, relu or raw factors): entries of a few dozen non-zero products,
  whose partial sums are as large as A.  The largest is 2^-22.70; four times that, rounded up to a power of two, is 2^-20.  The
  factor four is the margin _persistent_items.py gives an emulation whose inner order (here: the 16 columns of a K block, which
  the MFMA sums in an order of its own) is not the hardware's.  The constant is never raised to fit a kernel's output.
  It was set from the emulation alone, before any kernel had been measured per element.  The GPU column of
  profiles/wgrad_elements_errors.txt was filled afterwards: the fp32 kernels reach 2^-21.90 at most, 1.74 times the emulation's
  largest value; a later kernel change that moves that column says whether the constant still rests on a measurement.
* The split kernel at W < 4 (a row of W + 1 slots no longer than its ring of four, the producers six slots ahead) was first read
  from the code only (every load is clamped, dead slots are zero columns); the 2 x 3 cases here are its first runs, and they
  pass (guard bands intact, 2^-17.3 of A).

Inputs (``case_data``): randn operands with graded power-of-two channel scales, s_ci = 2^-(2 (ci mod 7)) on x and
s_co = 2^-(3 (co mod 5)) on gy, so that dW's entries span 2^-24 ... 1 and an error the size of a LARGE channel's rounding is a
gross error in a small one (``prev`` is graded the same way, or its 2^-24 |prev| would hide the small entries); a sprinkling of
factor-source entries (x itself in the self mode) overwritten with +0.0, -0.0 and 2^-149; sample 1 all zeros.
"""
import functools
import math
import os
import re

import torch
import torch.nn.functional as F

import _persistent_items as P

C_WGRAD_BF16X3 = P.C_BF16X3
C_WGRAD_F32 = 2.0 ** -20
U32 = 2.0 ** -24
WG_MAX = P.WG_MAX
TINY = 2.0 ** -149
MAX_NORM = {"f32": 2e-5, "bf16x3": 5e-5}          # the tensor-wide checks these tests tighten; asserted unchanged next to them

FMODES = ("none", "relu", "tanh", "raw", "self")
SPLIT_FMODES = ("none", "relu", "bits", "self")


# ---------------------------------------------------------------------------------------------------------------------------
# Shape rules of cmf_conv_tangent_wgrad (conv_wgrad.hip) and engine.conv_tangent_wgrad, mirrored
def family(cin, cout, taps, nc, fmode="none", f_group=1, precision="f32"):
    """The kernel family a launch reaches: 'split', 'thin3x3_nt1' .. 'thin3x3_nt4', 'thin1x1', 'rows3x3', 'general1x1'."""
    if (precision == "bf16x3" and taps == 9 and cin % 64 == 0 and cout % 64 == 0 and nc % 32 == 0
            and fmode in SPLIT_FMODES and f_group <= 1):
        return "split"
    assert fmode != "bits", "bit-mask factors are read by the split kernel only"
    if taps == 9 and cin * 9 <= 64:
        return f"thin3x3_nt{(cin * 9 + 15) // 16}"
    if taps == 1 and cout <= 16:
        return "thin1x1"
    return "rows3x3" if taps == 9 else "general1x1"


#: the lines of the dispatch that ``family`` mirrors: a rule change has to come through here (tests/test_wgrad_elements_host.py)
DISPATCH_LINES = {
    "conv_wgrad.hip": [
        "const bool thin_in = a->taps == 9 && a->cin * 9 <= 64 && !simple, thin_out = a->taps == 1 && a->cout <= 16;",
        "const int nt = thin_in ? (a->cin * 9 + 15) / 16 : 4;",
        ": nt == 1 ? (const void*)conv_wgrad_thin_kernel<9, 4, 1>",
        ": nt == 2 ? (const void*)conv_wgrad_thin_kernel<9, 4, 2>",
        ": (const void*)conv_wgrad_thin_kernel<9, 4, 4>;",
        "const int tgrid = (int)(nkb < 8 * WG_MAX ? (nkb + 7) / 8 : WG_MAX);",
        "const long long units = (a->taps == 9 && !simple) ? nrows : nkb;",
        "const int grid = (int)(units < WG_MAX ? units : WG_MAX);",
        "constexpr int WG_MAX = 256;",
    ],
    "conv_wgrad_bf16x3.hip": [
        "if (a->taps != 9 || a->cin % 64 || a->cout % 64 || a->nc <= 0 || a->nc % 32) return CMF_EINVAL;",
        "int wgp = nprob == 1 ? (int)(nrows < WG_MAX ? nrows : WG_MAX) : (WG_MAX / nprob) & ~7;",
    ],
    "../engine.py": [
        "split = ((precision or cfg().tangent) == \"bf16x3\" and taps == 9 and cin % 64 == 0 and cout % 64 == 0 and nc % 32 == 0",
        "and fmode in (F_NONE, F_RELU, F_SELF_RELU, F_RELU_BITS) and f_group <= 1)",
    ],
}


def missing_dispatch_lines():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cmf_amd", "csrc")
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    out = []
    for name, lines in DISPATCH_LINES.items():
        with open(os.path.join(root, name)) as fh:
            text = squeeze(fh.read())
        out += [(name, ln) for ln in lines if squeeze(ln) not in text]
    return out


class Case:
    """One launch: shape, factor mode, layout; ``nprob`` > 0: a batched launch of that many problems."""

    def __init__(self, precision, cin, cout, H, W, nc, taps=9, fmode="none", layout="panel", np_=3, f_group=1, nprob=0):
        self.precision, self.cin, self.cout, self.H, self.W, self.nc, self.taps = precision, cin, cout, H, W, nc, taps
        self.fmode, self.layout, self.np, self.f_group, self.nprob = fmode, layout, np_, f_group, nprob
        self.k = 3 if taps == 9 else 1
        self.family = family(cin, cout, taps, nc, fmode, f_group, precision)
        self.arithmetic = "bf16x3" if self.family == "split" else "f32"
        self.R = np_ * H * W * nc

    @property
    def id(self):
        return (f"{self.family}-ci{self.cin}-co{self.cout}-{self.H}x{self.W}-nc{self.nc}-{self.fmode}"
                + (f"-fg{self.f_group}" if self.f_group > 1 else "") + (f"-x{self.nprob}" if self.nprob else "") + f"-{self.layout}")

    def geometry(self):
        """(order, workgroups, waves that split a workgroup's K blocks) of the launch; one problem's share for a batch."""
        nsl = self.nc // 16
        nkb, nrows = self.np * self.H * self.W * nsl, self.np * self.H * nsl
        if self.family == "split":
            rows = P.wgrad_rows_split(self.H, self.nc, self.np)
            return "xcd_rows", ((WG_MAX // self.nprob) & ~7) if self.nprob > 1 else min(rows, WG_MAX), 1
        if self.family.startswith("thin"):
            return "blocks", (nkb + 7) // 8 if nkb < 8 * WG_MAX else WG_MAX, 8
        if self.family == "rows3x3":
            return "rows", min(nrows, WG_MAX), 1
        return "blocks", min(nkb, WG_MAX), 1


def _cases():
    out = []
    lay = lambda i: ("panel", "slice")[i % 2]
    rows = [(64, 64, 14, 14, 16), (17, 40, 5, 7, 32), (130, 70, 2, 4, 16), (64, 64, 1, 9, 16), (32, 16, 2, 1, 16), (16, 64, 3, 2, 16),
            (8, 8, 4, 3, 32)]
    for i, s in enumerate(rows):
        for j, fm in enumerate(FMODES):
            out.append(Case("f32", *s, fmode=fm, layout=lay(i + j)))
    out.append(Case("f32", 64, 64, 14, 14, 16, fmode="relu", layout="slice", f_group=16))
    # thin 3x3: every cin 1 .. 7 meets every factor mode and each of (cout 64 | 24) x (5 x 6 | 8 x 8); cin 3 on a one-row image
    thin = [(64, 5, 6), (24, 8, 8), (64, 8, 8), (24, 5, 6), (64, 5, 6)]
    for cin in range(1, 8):
        for j, fm in enumerate(FMODES):
            co, H, W = thin[(j + cin) % 5]
            out.append(Case("f32", cin, co, H, W, 16, fmode=fm, layout=lay(cin + j)))
    for j, fm in enumerate(FMODES):
        out.append(Case("f32", 3, 64, 1, 3, 16, fmode=fm, layout=lay(j)))
    for i, s in enumerate([(130, 12, 3, 9, 16), (64, 2, 4, 4, 16), (10, 16, 1, 5, 16), (10, 17, 1, 5, 16), (130, 70, 1, 37, 16)]):
        out.append(Case("f32", *s, taps=1, layout=lay(i)))
    split = [(64, 64, 14, 14, 32), (128, 64, 4, 8, 32), (64, 128, 2, 14, 64), (64, 64, 1, 5, 32), (64, 64, 2, 3, 32)]
    for i, s in enumerate(split):
        for j, fm in enumerate(SPLIT_FMODES):
            out.append(Case("bf16x3", *s, fmode=fm, layout=lay(i + j)))
    return out


CASES = _cases()
BATCHED = [Case("bf16x3", 64, 64, H, W, 32, fmode=("none", "self")[i % 2], layout="grouped", nprob=n)
           for i, (n, (H, W)) in enumerate((n, hw) for hw in ((4, 14), (2, 3)) for n in (1, 3, 16))]


# ---------------------------------------------------------------------------------------------------------------------------
# Inputs
def scales(cin, cout):
    return 2.0 ** (-2.0 * (torch.arange(cin) % 7)), 2.0 ** (-3.0 * (torch.arange(cout) % 5))


def _sprinkle(t, gen):
    """Every ~11th entry of ``t`` <- +0.0, -0.0, 2^-149 in turn."""
    flat = t.reshape(-1)
    idx = torch.randperm(flat.numel(), generator=gen)[:max(3, flat.numel() // 11)]
    flat[idx] = torch.tensor([0.0, -0.0, TINY]).repeat(-(-idx.numel() // 3))[:idx.numel()]
    return t


class Data:
    pass


def factor32(fmode, src):
    """The multiplier the kernels form from a factor source, in their fp32 arithmetic (tanh: 1 - f f; the rounding of f f and of
    the subtraction is part of what the bound covers)."""
    if fmode in ("relu", "bits"):
        return (src > 0).float()
    if fmode == "tanh":
        return 1.0 - src * src
    return src


def make_data(case, seed=0, graded=True):
    """x (np, cin, H, W, nc), gy (np, cout, H, W, nc), src (np, cin, H, W) or None, prev (cout, cin, k, k): float32.  ``graded``
    False: the same draws with every channel scale 1 (the channel-isolation check)."""
    d = Data()
    c = case
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * c.cin + 104729 * c.cout + 31 * c.H + 17 * c.W + c.nc + c.taps)
    d.s_ci, d.s_co = scales(c.cin, c.cout)
    x = torch.randn(c.np, c.cin, c.H, c.W, c.nc, generator=gen)
    gy = torch.randn(c.np, c.cout, c.H, c.W, c.nc, generator=gen)
    p = torch.randn(c.np, c.cin, c.H, c.W, generator=gen)
    prev = 4 * torch.randn(c.cout, c.cin, c.k, c.k, generator=gen)
    if graded:
        x, gy = x * d.s_ci.view(1, -1, 1, 1, 1), gy * d.s_co.view(1, -1, 1, 1, 1)
        prev = prev * d.s_co.view(-1, 1, 1, 1) * d.s_ci.view(1, -1, 1, 1)
    d.src = None
    if c.fmode == "self":
        _sprinkle(x, gen)
    elif c.fmode != "none":
        d.src = _sprinkle(torch.tanh(p) if c.fmode == "tanh" else p, gen)
    if c.np >= 3:
        x[1] = 0
    d.x, d.gy, d.prev = x, gy, prev
    d.xe = torch.relu(x) if c.fmode == "self" else x                       # what the factor multiplies
    d.fac32 = None if d.src is None else factor32(c.fmode, d.src)
    d.fac64 = None
    if d.src is not None:                                                  # float64 of THAT source: [f > 0], 1 - f^2, f
        s = d.src.double()
        d.fac64 = (s > 0).double() if c.fmode in ("relu", "bits") else 1 - s * s if c.fmode == "tanh" else s
    return d


@functools.lru_cache(maxsize=None)
def _case_data(case, seed):
    d = make_data(case, seed)
    d.want, d.A = reference(d.xe, d.gy, d.fac64, d.prev)
    return d


def case_data(case, seed=0):
    """The graded inputs of ``case`` with their float64 (want, A): computed once, shared, not to be modified."""
    return _case_data(case, seed)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference
def _cols(t):
    n, C, H, W, nc = t.shape
    return t.permute(0, 4, 1, 2, 3).reshape(n * nc, C, H, W)


def _dw(x, gy, k):
    out = torch.zeros(gy.shape[1], x.shape[1] * k * k, dtype=torch.float64)
    for n in range(x.shape[0]):                                            # per sample: the unfolded operand is 9 x the input
        u = F.unfold(_cols(x[n:n + 1]), k, padding=k // 2)                 # (nc, cin k k, HW)
        out += torch.einsum("bop,bkp->ok", _cols(gy[n:n + 1]).flatten(2), u)
    return out.view(gy.shape[1], x.shape[1], k, k)


def reference(x, gy, fac, prev):
    """float64 (want, A):  want = prev + dW,  A = sum |gy| |F x|,  both (cout, cin, k, k); ``fac`` (np, cin, H, W) or None
    multiplies x (for the self mode pass relu(x))."""
    k = prev.shape[-1]
    fx = x.double() if fac is None else x.double() * fac.double().unsqueeze(-1)
    return prev.double() + _dw(fx, gy.double(), k), _dw(fx.abs(), gy.double().abs(), k)


def bound(want, A, prev, c):
    return c * A + U32 * (prev.double().abs() + want.abs())


def ratio_over_A(got, want, A, prev):
    """max over the entries of (|got - want| - 2^-24 (|prev| + |want|)) / A, floored at 0; inf where A == 0 and got != prev."""
    err = ((got.double() - want).abs() - U32 * (prev.double().abs() + want.abs())).clamp_min(0)
    r = torch.where(A > 0, err / A.clamp_min(1e-300), torch.where(got.double() != prev.double(), torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max())


def max_norm_error(got, want, prev):
    """The tensor-wide figure of the older tests: max |dW_got - dW_want| / max |dW_want|."""
    dw = want - prev.double()
    return float(((got.double() - prev.double()) - dw).abs().max() / dw.abs().max().clamp_min(1e-30))


def log2(v):
    return math.log2(max(v, 1e-300))


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 emulation in the kernels' order
def _units(x, gy, fac, k, kc, leak_channels=None):
    """K blocks in (sample, pixel, slice) order: G (U, cout, kc), Pm (U, cin k k, kc) float32; kc columns per block."""
    n, cin, H, W, nc = x.shape
    fx = x if fac is None else x * fac.unsqueeze(-1)
    u = F.unfold(_cols(fx), k, padding=k // 2).reshape(n, nc, cin, k * k, H * W)
    if leak_channels is not None:                                          # injected defect (b), tests/test_wgrad_elements_host.py
        flat = _cols(fx).reshape(n, nc, cin, H * W)
        for dy in range(3):
            for y in range(H):
                src = (y + dy - 1) * W - 1                                 # the pixel "left of" column 0 in memory order
                if 0 <= src < H * W:
                    u[:, :, leak_channels, dy * 3, y * W] = flat[:, :, leak_channels, src]
    Pm = u.reshape(n, nc // kc, kc, cin * k * k, H * W).permute(0, 4, 1, 3, 2).reshape(-1, cin * k * k, kc)
    G = gy.reshape(n, gy.shape[1], H * W, nc // kc, kc).permute(0, 2, 3, 1, 4).reshape(-1, gy.shape[1], kc)
    return G.contiguous(), Pm.contiguous()


def _work_lists(order, n_wg, waves, np_, H, W, nsl):
    """Per accumulator (workgroup, or workgroup x wave) the K blocks it sums, in its order; block index = (sample HW + px) nsl + sl."""
    row = lambda n, y, sl: [((n * H + y) * W + xx) * nsl + sl for xx in range(W)]
    if order == "blocks":
        nkb = np_ * H * W * nsl
        per = -(-nkb // n_wg)
        return [list(range(min(nkb, b * per) + w, min(nkb, (b + 1) * per), waves)) for b in range(n_wg) for w in range(waves)]
    nrows = np_ * H * nsl
    if order == "rows":                                                    # row id = (sample H + y) nsl + slice, contiguous ranges
        per = -(-nrows // n_wg)
        return [sum((row(r // nsl // H, r // nsl % H, r % nsl) for r in range(min(nrows, b * per), min(nrows, (b + 1) * per))), [])
                for b in range(n_wg)]
    assert order == "xcd_rows"                                             # row id = (sample nsp + pair) H + y, dealt XCD-aware
    return [sum((row(r // H // nsl, r % H, r // H % nsl) for r in rows), []) for rows in P.xcd_walk(nrows, n_wg)]


def reduce_partials(ws):
    """wgrad_reduce_kernel: eight interleaved chains over the workgroups' blocks, the rest on chain 0, a fixed tree."""
    nwg = ws.shape[0]
    s8 = [torch.zeros_like(ws[0]) for _ in range(8)]
    g = 0
    while g + 8 <= nwg:
        for j in range(8):
            s8[j] = s8[j] + ws[g + j]
        g += 8
    while g < nwg:
        s8[0] = s8[0] + ws[g]
        g += 1
    return ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]))


def emulate(x, gy, fac, arithmetic, n_wg, order="blocks", waves=1, taps=9, drop_hi_lo=False, leak_channels=None):
    """float32 dW (cout, cin, k, k) in the kernels' order: every workgroup (``order``: 'blocks' = contiguous ranges of
    ceil(units / n_wg) K blocks in (sample, y, x, slice) order, split over ``waves`` waves that are summed in wave order; 'rows' /
    'xcd_rows' = image rows as the row-walking / the split kernel deal them) keeps one fp32 chain over its K blocks of 16 (split: 32)
    columns, then ``reduce_partials``.  "f32": exact products; "bf16x3": hi lo + lo hi + hi hi of ``_persistent_items.split``
    (``drop_hi_lo``: injected defect).  The caller adds the result to ``prev`` in fp32, as the reduction's ``+=`` does."""
    k = 3 if taps == 9 else 1
    n, cin, H, W, nc = x.shape
    kc = 32 if order == "xcd_rows" else 16
    G, Pm = _units(x, gy, fac, k, kc, leak_channels)
    lists = _work_lists(order, n_wg, waves, n, H, W, nc // kc)
    assert sorted(sum(lists, [])) == list(range(G.shape[0]))               # every K block exactly once
    L = max(len(l) for l in lists)
    idx = torch.tensor([l + [-1] * (L - len(l)) for l in lists], dtype=torch.long).reshape(len(lists), L)
    if arithmetic == "bf16x3":
        (gh, gl), (ph, pl) = P.split(G, torch.bfloat16, 2), P.split(Pm, torch.bfloat16, 2)
        terms = [(gh, pl), (gl, ph), (gh, ph)][1 if drop_hi_lo else 0:]
    else:
        terms = [(G, Pm)]
    acc = torch.zeros(len(lists), G.shape[1], Pm.shape[1])
    for j in range(L):
        live = (idx[:, j] >= 0).nonzero().reshape(-1)
        sel = idx[live, j]
        a = acc[live]
        for g_, p_ in terms:
            a = a + torch.bmm(g_[sel], p_[sel].transpose(1, 2))
        acc[live] = a
    if waves > 1:                                                          # thin kernels: the waves' blocks summed through LDS
        part = acc.view(n_wg, waves, *acc.shape[1:])
        acc = torch.zeros_like(part[:, 0])
        for w in range(waves):
            acc = acc + part[:, w]
    return reduce_partials(acc).view(G.shape[1], cin, k, k)


def emulate_case(case, d, **defect):
    order, n_wg, waves = case.geometry()
    return emulate(d.xe, d.gy, d.fac32, case.arithmetic, n_wg, order, waves, case.taps, **defect)


def c_of(case):
    return C_WGRAD_BF16X3 if case.arithmetic == "bf16x3" else C_WGRAD_F32


def check_elements(label, got, want, A, prev, arithmetic, R, tag="WGRAD_ELEMENTS"):
    """The assertions every weight-gradient result gets (CPU tensors): finite; A == 0 entries untouched; every entry within
    c A + 2^-24 (|prev| + |want|) and, for exact products, within the rigorous (R + 9) 2^-24 A; the older tensor-wide bound.
    Prints and returns max err / A."""
    c = C_WGRAD_BF16X3 if arithmetic == "bf16x3" else C_WGRAD_F32
    got, prev = got.detach().cpu(), prev.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{label}: non-finite entries"
    dead = A == 0
    assert torch.equal(got[dead], prev[dead]), f"{label}: entries without a non-zero product must keep prev bit for bit"
    ratio, rel = ratio_over_A(got, want, A, prev), max_norm_error(got, want, prev)
    print(f"\n{tag} {label}: max |err| / A = 2^{log2(ratio):.2f} (c = 2^{log2(c):.0f})  max-norm error {rel:.2e} "
          f"(bound {MAX_NORM[arithmetic]:.0e})  A == 0 at {int(dead.sum())} of {dead.numel()} entries")
    err = (got.double() - want).abs()
    bad = err > bound(want, A, prev, c)
    assert not bool(bad.any()), (f"{label}: {int(bad.sum())} entries beyond c A + 2^-24 (|prev| + |want|), first (co, ci, ky, kx) "
                                 f"{bad.nonzero()[:5].tolist()}; max err / A = 2^{log2(ratio):.2f}, c = 2^{log2(c):.0f}")
    if arithmetic == "f32":
        assert not bool((err > bound(want, A, prev, (R + 9) * U32)).any()), f"{label}: beyond the rigorous (R + 9) 2^-24 A"
    assert rel < MAX_NORM[arithmetic], (label, rel)
    return ratio
