"""Helpers shared by tests/test_gpu_mlp_coupler_elements.py and tests/test_mlp_coupler_elements_host.py (not collected by pytest).

The fused MLP coupling layer (cmf_amd/csrc/mlp_coupler.hip: mlp_coupler_kernel<HT, TAN, NW>, mlp_coupler_split_kernel,
pack_mlp_layer_kernel) against a float64 model of ONE coupling layer, PER ELEMENT:

    |got - want| <= bound,     bound from the float64 model and the fp32 inputs alone, never from a kernel's output.

The model (``model``) follows the kernel file's header: a tanh MLP with the tanh rule for the Jacobian columns and a linear last
layer (t, s) = W h + b,
    h' = tanh(W h + b),   hdot' = (1 - h'^2) (W hdot)
    decode  x = z e^{-s} - t,   xdot = e^{-s} (v - z sdot) - tdot        (PRIMAL mode: lj -= sum s)
    encode  z = (x + t) e^{s},  lj += sum s

The bound is carried through that model next to every value, element by element.  u = 2^-24 (fp32, round to nearest); e_x is the
bound on |kernel's x - model's x|.  Every rounding site adds its own first-order term (the cross terms e e' are kept where they
cost nothing):

* dot product  a = W h + b  (tangent columns: no bias):   e_a = c (|W| (|h| + e_h) + |b|) + |W| e_h,   c = min(c_dot, (K + 1) u)
  per output row, K = the row's non-zero weights.  (K + 1) u is the rigorous bound of ANY order of K exact products, K - 1
  additions and the bias addition, so it is the ceiling of the constant: a row of four weights never gets more than 5 u.
* tanh is 1-Lipschitz: it passes e_a on, and the device's tanhf adds c_tanh u |h|.
* g = 1 - h^2:   e_g = 2 |h| e_h + e_h^2 + 2 u   (the rounded square and the rounded difference, both of values <= 1).
* hdot' = g adot:   e = |g| e_ad + |adot| e_g + e_ad e_g, then one rounding u (|hdot'| + e).
* exp:   e_E = E (expm1(e_s) + c_exp u e^{e_s}),  E = e^{-s} or e^{s}: the propagated bound of s, then expf's own error.
* every product and every sum of the coupling update: the propagated bounds of its operands, then one rounding u (|value| + e).
  (The compiler contracts some of them into fused multiply-adds: fewer roundings, never more.)
* sum s over the n_mod modified elements: sum e_s + depth u sum (|s| + e_s), depth = the additions one term passes through in the
  kernel's reduction (per-wave kernels: a chain of ceil(n_mod / 4) per lane group, two shuffle steps; split kernel: a chain of
  ceil(n_mod / 32), two shuffle steps, a chain over the eight waves' partial sums).
* the final  lj +=  : u (|prev| + |want|), as in tests/_wgrad_elements.py.

The constants.
* ``C_DOT``: from a CPU emulation of the kernels' summation order (``emulate``): per-wave kernels one fp32 chain, K-group-major then
  the four K-steps of a group, every K-step (one v_mfma_f32_16x16x4_f32: four exact products, one per lane group kq) taken as four
  chained fused multiply-adds, then the bias; the split kernel two interleaved chains (K-steps 0, 2 and 1, 3 of every group) and
  acc0 + acc1 + bias.  The largest |emulated - exact| / (|W| |h| + |b|) over every dot product of every case's own inputs
  (tests/test_mlp_coupler_elements_host.py prints it; profiles/mlp_coupler_errors.txt keeps it), times four, rounded up to a power
  of two.  The factor four is the margin tests/_persistent_items.py gives an emulation whose inner order (here: the four products
  of one MFMA K-step) is not the hardware's.  One constant per kernel and hidden tile count HT (the template instances
  differ in the length of a hidden layer's chain: 16, 32, 128 K positions).  Measured: per-wave kernels HT = 1 2^-22.34, HT = 2
  2^-21.73 (a 20-term chain of the [1, 20, 4] network: 4.8 u), HT = 8 2^-22.03; split kernel 2^-22.58: C_DOT = 2^-20, 2^-19,
  2^-20, 2^-20.  Rows of fewer than 15 (31) weights are held to their ceiling (K + 1) u instead.
* ``C_TANH`` = 5 and ``C_EXP`` = 3: the single-precision ulp limits the OpenCL specification sets for tanh and exp, which the
  device math library is built to meet.  They are NOT measured here and cannot be derived here: they are the documented contract
  of tanhf / expf that this bound takes on trust.
* No constant is ever raised to fit a kernel's output.

Inputs (``case_data``), chosen so that the bound means something.  A worst-case bound grows by the absolute row sum of |W| per
layer: dense N(0, 1.5^2 / K) weights through four 128-wide layers make it as large as the values themselves, and such a test
passes anything.  So networks with more than one hidden layer wider than 32 get SPARSE rows -- four non-zero weights N(0, 0.6^2)
per row, the first at input (row mod K) so that 128 rows touch every K position of every packed image, the others at random
inputs -- and networks with one hidden layer or hidden widths <= 32 get dense N(0, 1.5^2 / K) weights.  The host test asserts
median(bound / |want|) < 1e-3 over the tangent outputs of every case.  Every seventh first-layer bias is +6 (saturated units,
1 - h^2 near 2^-16, where fp32's 1 - h h cancels); the last layer's log-scale biases spread s over about +-3; tangent column j is
scaled by 2^-(3 j), so that an error the size of column 0's rounding is gross in column 10; lj starts non-zero.
"""
import functools
import math
import os
import re

import numpy as np
import torch

U32 = 2.0 ** -24
C_TANH = 5.0
C_EXP = 3.0
C_DOT = {"wave1": 2.0 ** -20, "wave2": 2.0 ** -19, "wave8": 2.0 ** -20, "split": 2.0 ** -20}
MAX_NORM = 5e-6                     # the tensor-wide check of tests/test_gpu_round2.py, asserted unchanged next to the bound
EMU_SAMPLES = 96                    # ``emulate`` runs the first and the last EMU_SAMPLES samples of a large batch


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# The dispatch of cmf_mlp_coupler (mlp_coupler.hip), mirrored
class Variant:
    def __init__(self, kernel, HT, NW, n_tiles, grid, lds, per_cu, spt):
        self.kernel, self.HT, self.NW, self.n_tiles, self.grid, self.lds, self.per_cu, self.spt = kernel, HT, NW, n_tiles, grid, lds, per_cu, spt

    @property
    def path(self):
        """(kernel, HT, NW, more tiles than workgroups)"""
        return self.kernel, self.HT, self.NW, self.n_tiles > self.grid

    def __repr__(self):
        return (f"{self.kernel} HT={self.HT} NW={self.NW} tiles={self.n_tiles} grid={self.grid} lds={self.lds} B "
                f"per_cu={self.per_cu} samples/tile={self.spt * self.NW if self.kernel != 'split' else 16}")


def hidden_tiles(hmax):
    return 1 if hmax <= 16 else (2 if hmax <= 32 else 8)


def layer_tiles(widths, HT):
    """(output tiles, input K groups) of every layer: hidden widths padded to HT tiles."""
    L = len(widths) - 1
    return [(ceil_div(widths[-1], 16) if l == L - 1 else HT, ceil_div(widths[0], 16) if l == 0 else HT) for l in range(L)]


def image_floats(n_mt, n_kg):
    return n_mt * n_kg * 256 + 16 * n_mt


def variant(widths, B, ncols, cus):
    """The kernel a launch of cmf_mlp_coupler reaches: ``widths`` = [cin, hidden ..., outputs], ``ncols`` None = PRIMAL mode."""
    HT = hidden_tiles(max(widths[1:-1]))
    buf = ceil_div(max(image_floats(mt, kg) for mt, kg in layer_tiles(widths, HT)), 256) * 256
    tan = ncols is not None
    if not tan and HT == 8 and B <= 128 * 2 * cus:
        n_tiles = ceil_div(B, 16)
        lds = (2 * buf + 2 * 8 * 64 * 4 + 64 * 16 + 8 * 16) * 4
        return Variant("split", 8, 8, n_tiles, min(n_tiles, cus), lds, 1, 16)
    spt = 16 // (ncols + 1) if tan else 16
    NW = 8
    if tan and ceil_div(B, 8 * spt) < cus and B > 4 * spt:
        NW = 4
    out_pad = ceil_div(widths[-1], 16) * 16
    scr = max(16 * out_pad, 128 * spt if tan else 0)
    lds = (2 * buf + NW * scr) * 4
    per_cu = 2 if lds <= 40 * 1024 else 1
    n_tiles = ceil_div(B, NW * spt)
    return Variant("tangent" if tan else "primal", HT, NW, n_tiles, min(n_tiles, cus * per_cu), lds, per_cu, spt)


#: the lines of the launcher that ``variant`` mirrors: a dispatch change has to come through here
DISPATCH_LINES = {
    "mlp_coupler.hip": [
        "extern \"C\" int cmf_mlp_hidden_tiles(int max_hidden_width) { return max_hidden_width <= 16 ? 1 : (max_hidden_width <= 32 ? 2 : 8); }",
        "__host__ __device__ inline long long image_floats(int n_kg, int n_mt) { return (long long)n_mt * n_kg * 256 + 16 * n_mt; }",
        "__host__ __device__ inline int layer_kg(const cmf_mlp_coupler_args& a, int l, int ht) { return l == 0 ? (a.width[0] + 15) / 16 : ht; }",
        "return l == a.n_layers - 1 ? (a.width[a.n_layers] + 15) / 16 : ht;",
        "buf = (buf + 255) / 256 * 256;",
        "const int spt = TAN ? 16 / (a.ncols + 1) : 16;",
        "const int per_tile = NW * spt;",
        "const int n_tiles = cmf_ceil_div(a.B, per_tile);",
        "if (n_tiles < cmf_device_cus() && a.B > 4 * spt) return launch<HT, TAN, 4>(a, buf_floats, s);",
        "const int out_pad = (a.width[a.n_layers] + 15) / 16 * 16;",
        "const int s_floats = TAN ? 128 * spt : 0;",
        "const int scr_floats = 16 * out_pad > s_floats ? 16 * out_pad : s_floats;",
        "const int lds = (2 * buf_floats + NW * scr_floats) * (int)sizeof(float);",
        "const int per_cu = lds <= 40 * 1024 ? 2 : 1;",
        "const int grid = n_tiles < cus * per_cu ? n_tiles : cus * per_cu;",
        "const int n_tiles = cmf_ceil_div(a.B, 16);",
        "const int lds = (2 * buf_floats + 2 * 8 * 64 * 4 + 64 * 16 + WAVES * 16) * (int)sizeof(float);",
        "const int grid = n_tiles < cus ? n_tiles : cus;",
        "if (ht == 1) return launch<1, true>(*a, (int)buf, s);",
        "if (ht == 2) return launch<2, true>(*a, (int)buf, s);",
        "return launch<8, true>(*a, (int)buf, s);",
        "if (ht == 1) return launch<1, false>(*a, (int)buf, s);",
        "if (ht == 2) return launch<2, false>(*a, (int)buf, s);",
        "if (a->B <= 128 * 2 * cmf_device_cus()) return launch_split(*a, (int)buf, s);",
        "return launch<8, false>(*a, (int)buf, s);",
        "constexpr int WAVES = 8;",
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


# ---------------------------------------------------------------------------------------------------------------------------
# The packed layer image (pack_mlp_layer_kernel), from the index formula in the comment above it
def pack_image(W, b, first, n_mt, n_kg):
    """A fragments [mt][kg][64 lanes][4] + bias [16 mt] as float32: fragment (mt, kg) of lane (kq = lane / 16, m = lane % 16),
    component j = the weight of output feature 16 mt + m and input feature 16 kg + 4 j + kq (first layer) or 16 kg + 4 kq + j
    (later layers); zero beyond the sizes.  ``b`` None: zero bias."""
    W = np.asarray(W, dtype=np.float32)
    out_f, in_f = W.shape
    nfrag = n_mt * n_kg * 256
    img = np.zeros(nfrag + 16 * n_mt, dtype=np.float32)
    i = np.arange(nfrag)
    j, lane, f = i & 3, (i >> 2) & 63, i >> 8
    kg, mt, kq, m = f % n_kg, f // n_kg, lane >> 4, lane & 15
    o = 16 * mt + m
    k = 16 * kg + 4 * j + kq if first else 16 * kg + 4 * kq + j
    ok = (o < out_f) & (k < in_f)
    img[i[ok]] = W[o[ok], k[ok]]
    if b is not None:
        img[nfrag:nfrag + out_f] = np.asarray(b, dtype=np.float32)
    return img


def unpack_image(img, first, n_mt, n_kg):
    """(W (16 n_mt, 16 n_kg), b (16 n_mt,)) read back fragment by fragment, in plain loops."""
    W = np.full((16 * n_mt, 16 * n_kg), np.nan, dtype=np.float32)
    for mt in range(n_mt):
        for kg in range(n_kg):
            for lane in range(64):
                kq, m = lane // 16, lane % 16
                for j in range(4):
                    k = 16 * kg + (4 * j + kq if first else 4 * kq + j)
                    W[16 * mt + m, k] = img[((mt * n_kg + kg) * 64 + lane) * 4 + j]
    return W, np.array(img[n_mt * n_kg * 256:], dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# Cases
class Case:
    """One coupling layer: D elements, the network reads ``pass_idx`` (an arithmetic progression: chan_off, chan_step, cin) and the
    layer modifies ``mod_idx``; ``ncols`` None = PRIMAL mode (both directions, with lj), else TANGENT mode decode; ``B(cus)``."""

    def __init__(self, id, D, pass_idx, mod_idx, hidden, ncols, B, path):
        self.id, self.D, self.hidden, self.ncols, self._B, self.want_path = id, D, list(hidden), ncols, B, path
        self.pass_idx, self.mod_idx = list(pass_idx), list(mod_idx)
        assert not set(self.pass_idx) & set(self.mod_idx) and max(self.pass_idx + self.mod_idx) < D
        self.cmod = len(self.mod_idx)
        self.widths = [len(self.pass_idx)] + self.hidden + [2 * self.cmod]
        wide = [h for h in self.hidden if h > 32]
        self.weights = "sparse" if len(self.hidden) > 1 and len(wide) > 1 else "dense"

    def B(self, cus):
        return self._B(cus) if callable(self._B) else self._B

    def variant(self, cus, ncols="own"):
        return variant(self.widths, self.B(cus), self.ncols if ncols == "own" else ncols, cus)

    @property
    def tangent(self):
        return self.ncols is not None

    @property
    def modes(self):
        return ("tangent", "decode") if self.tangent else ("decode", "encode")

    def __hash__(self):
        return hash(self.id)

    def __eq__(self, other):
        return self.id == other.id


def _cases():
    r = lambda a, b, s=1: list(range(a, b, s))
    out = [Case("tan-ht1-nw4-ragged", 3, [1], [0, 2], [10, 10], 1, 37, ("tangent", 1, 4, False))]
    for nc in (2, 3, 4, 5, 7, 8):                                          # 5, 4, 3, 2, 2, 1 samples per tile
        spt = 16 // (nc + 1)
        p, m = (r(0, 6, 2), r(1, 6, 2)) if nc % 2 == 0 else (r(1, 6, 2), r(0, 6, 2))
        out.append(Case(f"tan-ht1-nw4-pack{nc}", 6, p, m, [10, 10], nc, 5 * spt + 1, ("tangent", 1, 4, False)))
    out += [
        Case("tan-ht2-nw8-dead-waves", 9, r(0, 9, 2), r(1, 9, 2), [32, 17], 15, 3, ("tangent", 2, 8, False)),
        Case("tan-ht2-nw8-percu2-multi", 3, [2], [0, 1], [20], 15, lambda cus: 16 * cus + 11, ("tangent", 2, 8, True)),
        Case("tan-ht8-nw4-multi-L3", 4, [1, 3], [0, 2], [128, 128], 15, lambda cus: 4 * cus + 5, ("tangent", 8, 4, True)),
        Case("tan-ht8-nw8-multi-L3", 4, [0, 1], [2, 3], [128, 128], 15, lambda cus: 8 * cus + 11, ("tangent", 8, 8, True)),
        Case("tan-ht8-cin21-L5", 43, r(1, 43, 2), r(0, 43, 4), [128] * 4, 10, 77, ("tangent", 8, 4, False)),
        Case("tan-ht8-cin128-dense", 132, r(4, 132), r(0, 4), [128], 10, 9, ("tangent", 8, 4, False)),
        Case("pri-ht1-two-tiles", 3, [0], [1, 2], [10, 10], None, 131, ("primal", 1, 8, False)),
        Case("pri-ht2-percu2-multi", 5, [1, 3], [0, 2, 4], [32], None, lambda cus: 256 * cus + 133, ("primal", 2, 8, True)),
        Case("split-one-ragged-tile", 64, r(0, 64, 2), r(1, 64, 2), [33], None, 5, ("split", 8, 8, False)),
        Case("split-multi-L5", 43, r(1, 43, 2), r(0, 43, 4), [128] * 4, None, lambda cus: 16 * cus + 19, ("split", 8, 8, True)),
        Case("split-multi-L2", 64, r(1, 64, 2), r(0, 64, 2), [100], None, lambda cus: 16 * cus + 19, ("split", 8, 8, True)),
        Case("pri-ht8-per-wave", 64, r(32, 64), r(0, 32), [33], None, lambda cus: 256 * cus + 133, ("primal", 8, 8, True)),
    ]
    return out


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------------------
# Inputs
def make_net(case, gen):
    """[(W (out, in), b (out,))] float32, see the module docstring."""
    net, L = [], len(case.widths) - 1
    for l in range(L):
        K, out = case.widths[l], case.widths[l + 1]
        if case.weights == "sparse" and K > 4:
            W = torch.zeros(out, K)
            pos = torch.rand(out, K, generator=gen)
            pos[torch.arange(out), torch.arange(out) % K] = 2.0            # the covering position first
            idx = pos.argsort(1, descending=True)[:, :4]
            W.scatter_(1, idx, 0.6 * torch.randn(out, 4, generator=gen))
        else:
            W = torch.randn(out, K, generator=gen) * (1.5 / math.sqrt(K))
        b = 0.3 * torch.randn(out, generator=gen)
        if l == 0:
            b[::7] = 6.0
        if l == L - 1:
            b[case.cmod:] = torch.linspace(-2.5, 2.5, case.cmod) if case.cmod > 1 else torch.tensor([1.5])
        net.append((W.contiguous(), b.contiguous()))
    return net


class Data:
    pass


def column_scales(ncols):
    return 2.0 ** (-3.0 * torch.arange(ncols))


@functools.lru_cache(maxsize=None)
def case_data(case, cus):
    """net, z (B, D), V (B, D, ncols) graded and Vu (unit column scales), lj0 (B,): float32, with the float64 ``model`` of every
    mode the GPU test runs (``d.ref``).  Computed once per (case, CU count), shared, not to be modified."""
    d = Data()
    B = case.B(cus)
    gen = torch.Generator().manual_seed(7919 * CASES.index(case) + 31)
    d.B, d.net = B, make_net(case, gen)
    d.z = torch.randn(B, case.D, generator=gen)
    d.lj0 = 1.0 + torch.randn(B, generator=gen)
    d.V = d.Vu = None
    if case.tangent:
        d.Vu = torch.randn(B, case.D, case.ncols, generator=gen)
        d.V = d.Vu * column_scales(case.ncols)
    # TANGENT cases also run the PRIMAL-mode decode of the same inputs (the split kernel where the hidden layers are wide)
    d.ref = {mode: model(case, d, mode, kernel_of(case, cus, mode)) for mode in case.modes}
    return d


def kernel_of(case, cus, mode):
    """'split' | 'wave1' | 'wave2' | 'wave8' (per-wave kernels by hidden tiles HT): the arithmetic (C_DOT, lj reduction) of the kernel that ``mode`` of ``case`` reaches."""
    v = case.variant(cus) if mode == "tangent" or not case.tangent else case.variant(cus, None)
    return "split" if v.kernel == "split" else f"wave{v.HT}"


# ---------------------------------------------------------------------------------------------------------------------------
# float64 model with its running bound
def _rounded(v, e):
    """Bound after one fp32 rounding of a value the kernel holds to within ``e`` of ``v``."""
    return e + U32 * (v.abs() + e)


def lj_depth(kernel, n_mod):
    return ceil_div(n_mod, 32) + 2 + 8 if kernel == "split" else ceil_div(n_mod, 4) + 2


def network(net, x, xd, c_dot):
    """(Y, E_Y) (B, 1 + nc, outputs) float64: column 0 the primal, columns 1 .. the Jacobian columns; x (B, cin), xd (B, nc, cin)."""
    X = x.double()[:, None, :] if xd is None else torch.cat([x.double()[:, None, :], xd.double()], 1)
    E = torch.zeros_like(X)
    for l, (W, b) in enumerate(net):
        W64, b64 = W.double(), b.double()
        Wa = W64.abs()
        c = torch.minimum(torch.full((W.shape[0],), float(c_dot), dtype=torch.float64), ((W != 0).sum(1) + 1).double() * U32)
        A = X @ W64.T
        M = (X.abs() + E) @ Wa.T
        A[:, 0] += b64
        M[:, 0] += b64.abs()
        EA = c * M + E @ Wa.T
        if l == len(net) - 1:
            return A, EA
        h = torch.tanh(A[:, 0])
        eh = EA[:, 0] + C_TANH * U32 * h.abs()
        g = 1 - h * h
        eg = 2 * h.abs() * eh + eh * eh + 2 * U32
        X, E = torch.empty_like(A), torch.empty_like(A)
        X[:, 0], E[:, 0] = h, eh
        Ad, EAd = A[:, 1:], EA[:, 1:]
        Hd = g[:, None] * Ad
        X[:, 1:] = Hd
        E[:, 1:] = _rounded(Hd, g.abs()[:, None] * EAd + Ad.abs() * eg[:, None] + EAd * eg[:, None])


class Ref:
    """want / bound of z (B, D), T (B, D, ncols) and lj (B,), float64; rows the layer does not modify: want = input, bound 0."""


def model(case, d, mode, kernel):
    """``mode``: 'tangent' (decode of z and the Jacobian columns, no lj), 'decode' / 'encode' (PRIMAL mode with lj);
    ``kernel``: ``kernel_of`` -- which C_DOT and which lj reduction depth."""
    r = Ref()
    mod, cm = case.mod_idx, case.cmod
    z = d.z.double()
    zp = z[:, case.pass_idx]
    vd = d.V.double().permute(0, 2, 1) if mode == "tangent" else None         # (B, nc, D)
    Y, EY = network(d.net, zp, None if vd is None else vd[:, :, case.pass_idx], C_DOT[kernel])
    t, s, et, es = Y[:, 0, :cm], Y[:, 0, cm:], EY[:, 0, :cm], EY[:, 0, cm:]
    zm = z[:, mod]
    sign = 1.0 if mode == "encode" else -1.0
    Ex = torch.exp(sign * s)
    eEx = Ex * (torch.expm1(es) + C_EXP * U32 * torch.exp(es))
    r.z, r.z_bound = z.clone(), torch.zeros_like(z)
    if mode == "encode":
        w = zm + t
        ew = _rounded(w, et)
        out = w * Ex
        eo = _rounded(out, w.abs() * eEx + Ex * ew + ew * eEx)
    else:
        p = zm * Ex
        ep = _rounded(p, zm.abs() * eEx)
        out = p - t
        eo = _rounded(out, ep + et)
    r.z[:, mod], r.z_bound[:, mod] = out, eo
    r.s = s
    r.T = r.T_bound = r.lj = r.lj_bound = None
    if mode == "tangent":
        td, sd, etd, esd = Y[:, 1:, :cm], Y[:, 1:, cm:], EY[:, 1:, :cm], EY[:, 1:, cm:]
        v = vd[:, :, mod]
        p = zm[:, None] * sd
        ep = _rounded(p, zm.abs()[:, None] * esd)
        q = v - p
        eq = _rounded(q, ep)
        rr = Ex[:, None] * q
        er = _rounded(rr, Ex[:, None] * eq + q.abs() * eEx[:, None] + eEx[:, None] * eq)
        xd = rr - td
        exd = _rounded(xd, er + etd)
        r.T, r.T_bound = vd.clone(), torch.zeros_like(vd)
        r.T[:, :, mod], r.T_bound[:, :, mod] = xd, exd
        r.T, r.T_bound = r.T.permute(0, 2, 1).contiguous(), r.T_bound.permute(0, 2, 1).contiguous()
    else:
        S = s.sum(1)
        eS = es.sum(1) + lj_depth(kernel, cm) * U32 * (s.abs() + es).sum(1)
        prev = d.lj0.double()
        r.lj = prev + sign * S
        r.lj_bound = eS + U32 * (prev.abs() + r.lj.abs())
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 emulation in the kernels' order
def emu_subset(B):
    """Sample indices ``emulate`` runs: all of a small batch, the first and last EMU_SAMPLES of a large one."""
    idx = torch.arange(B)
    return idx if B <= 2 * EMU_SAMPLES else torch.cat([idx[:EMU_SAMPLES], idx[-EMU_SAMPLES:]])


def k_steps(n_kg, first):
    """Input feature of lane group kq in K-step (kg, j), in the order the MFMAs are issued: [(kg, j, [k of kq 0 .. 3])]."""
    return [(kg, j, [16 * kg + (4 * j + kq if first else 4 * kq + j) for kq in range(4)]) for kg in range(n_kg) for j in range(4)]


def emu_dot(W, b, X, first, n_kg, kernel):
    """fp32 X (n, in) W^T + b in the kernel's order; ``b`` None: no bias (tangent columns)."""
    n, K = X.shape
    W64, X64 = W.double(), X.double()
    acc = [torch.zeros(n, W.shape[0]), torch.zeros(n, W.shape[0])]
    for kg, j, ks in k_steps(n_kg, first):
        a = (j & 1) if kernel == "split" else 0
        for k in ks:
            if k < K:
                acc[a] = (acc[a].double() + X64[:, k, None] * W64[None, :, k]).float()
    y = acc[0] + acc[1] if kernel == "split" else acc[0]
    return y if b is None else y + b


def emu_lj(s, kernel):
    """sum of s (n, n_mod) float32 in the kernels' reduction order."""
    n, nm = s.shape
    step = 32 if kernel == "split" else 4
    part = torch.zeros(n, step)
    for e0 in range(0, nm, step):
        w = min(step, nm - e0)
        part[:, :w] = part[:, :w] + s[:, e0:e0 + w]
    part = part.view(n, step // 4, 4)                                      # [wave][kq]
    tot = (part[:, :, 0] + part[:, :, 1]) + (part[:, :, 2] + part[:, :, 3])
    if kernel != "split":
        return tot[:, 0]
    t = torch.zeros(n)
    for w in range(8):
        t = t + tot[:, w]
    return t


class Emu:
    pass


def emulate(case, d, mode, kernel, idx=None, net=None):
    """The whole layer in fp32 in the kernels' order on the samples ``idx`` (default ``emu_subset``): z, T, lj as the kernel would
    leave them (CPU tanh / exp for the device's), and ``dot_ratio`` / ``dot_ceiling``: the largest |emulated - exact| /
    (|W| |x| + |b|) over every dot product (exact = float64 on the SAME fp32 operands), and the largest of that error over the
    rigorous (K + 1) u (|W| |x| + |b|).  ``net``: other weights than the case's (injected defects)."""
    e = Emu()
    idx = emu_subset(d.B) if idx is None else idx
    net = d.net if net is None else net
    mod, cm = case.mod_idx, case.cmod
    z = d.z[idx].clone()
    n = z.shape[0]
    nc = case.ncols if mode == "tangent" else 0
    X = z[:, case.pass_idx][:, None, :]
    if nc:
        X = torch.cat([X, d.V[idx].permute(0, 2, 1)[:, :, case.pass_idx]], 1)
    X = X.contiguous()
    HT = hidden_tiles(max(case.widths[1:-1]))
    e.dot_ratio = e.dot_ceiling = 0.0
    for l, ((W, b), (n_mt, n_kg)) in enumerate(zip(net, layer_tiles(case.widths, HT))):
        flat = X.reshape(n * (1 + nc), -1)
        A = emu_dot(W, None, flat, l == 0, n_kg, kernel).view(n, 1 + nc, -1)
        A[:, 0] = A[:, 0] + b
        exact = flat.double() @ W.double().T
        mag = flat.double().abs() @ W.double().abs().T
        exact, mag = exact.view(n, 1 + nc, -1), mag.view(n, 1 + nc, -1)
        exact[:, 0] += b.double()
        mag[:, 0] += b.double().abs()
        err = (A.double() - exact).abs()
        live = mag > 0
        e.dot_ratio = max(e.dot_ratio, float((err[live] / mag[live]).max()))
        ceil = ((W != 0).sum(1) + 1).double() * U32 * mag
        e.dot_ceiling = max(e.dot_ceiling, float((err[live] / ceil[live]).max()))
        assert bool((err[~live] == 0).all())
        if l == len(net) - 1:
            Y = A
            break
        h = torch.tanh(A[:, 0])
        X = torch.empty_like(A)
        X[:, 0] = h
        X[:, 1:] = A[:, 1:] * (1.0 - h * h)[:, None]
    t, s = Y[:, 0, :cm], Y[:, 0, cm:]
    zm = z[:, mod]
    e.T = e.lj = None
    if mode == "encode":
        z[:, mod] = (zm + t) * torch.exp(s)
    else:
        es = torch.exp(-s)
        z[:, mod] = zm * es - t
        if nc:
            T = d.V[idx].clone()
            sd, td = Y[:, 1:, cm:].permute(0, 2, 1), Y[:, 1:, :cm].permute(0, 2, 1)     # (n, cm, nc)
            T[:, mod] = es[:, :, None] * (T[:, mod] - zm[:, :, None] * sd) - td
            e.T = T
    if mode != "tangent":
        S = emu_lj(s.contiguous(), kernel)
        e.lj = d.lj0[idx] + (S if mode == "encode" else -S)
    e.z, e.idx = z, idx
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# The assertions every result gets
def rel(a, b, floor=1e-9):
    """The tensor-wide figure of the older tests (tests/test_gpu_parity.py ``rel``)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(floor))


def err_over_bound(got, want, bound):
    """max |got - want| / bound; where bound == 0 (elements the layer does not touch) any difference counts as inf."""
    err = (got.double() - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def check_elements(label, ref, z, T=None, lj=None, idx=None, tag="MLP_COUPLER_ELEMENTS", norm=True):
    """z (n, D), T (n, D, ncols), lj (n,) float32 on the CPU against ``ref`` (rows ``idx`` of it): finite, every element within its
    bound, the older tensor-wide 5e-6 next to it.  Prints and returns {name: max err / bound}."""
    sel = (lambda t: t) if idx is None else (lambda t: t[idx])
    out = {}
    for name, got, want, bound in (("z", z, ref.z, ref.z_bound), ("T", T, ref.T, ref.T_bound), ("lj", lj, ref.lj, ref.lj_bound)):
        if got is None:
            continue
        assert want is not None, (label, name)
        got, want, bound = got.detach().cpu(), sel(want), sel(bound)
        assert bool(torch.isfinite(got).all()), f"{label}: non-finite {name}"
        out[name] = err_over_bound(got, want, bound)
        bad = (got.double() - want).abs() > bound
        rl = rel(got, want)
        print(f"\n{tag} {label} {name}: max err / bound = {out[name]:.3f}  tensor-wide error {rl:.2e} (bound {MAX_NORM:.0e})")
        assert not bool(bad.any()), (f"{label}: {int(bad.sum())} elements of {name} beyond the per-element bound, first "
                                     f"{bad.nonzero()[:5].tolist()}; max err / bound = {out[name]:.3f}")
        if norm:
            assert rl < MAX_NORM, (label, name, rl)
    return out


def bound_over_value(ref, case):
    """median of bound / |want| over the tangent outputs (PRIMAL cases: over the modified z)."""
    if ref.T is not None:
        w, b = ref.T[:, case.mod_idx], ref.T_bound[:, case.mod_idx]
    else:
        w, b = ref.z[:, case.mod_idx], ref.z_bound[:, case.mod_idx]
    return float((b / w.abs().clamp_min(1e-300)).median())
