"""The Jacobian head at every Gram / Cholesky width class, per element (``-m gpu``).

``cmf_gram_cholesky`` dispatches to five kernels (cmf_gram_cholesky_family); every case here asserts the family before it launches,
launches THROUGH THE C ABI with explicit strides, and holds every output element to a bound relative to float64 that comes from a
CPU emulation of the arithmetic (tests/_gram_head.py, checked without a GPU by tests/test_gram_head_host.py):

* Gram ``|G - G64| <= C_GRAM A`` with ``A = |J|^T |J|``; the L1 terms against float64 sums with a bound from the same constant plus
  the float32 summation depth; log-det per sample ``<= C_LOGDET (sum |G^-1| A + sum |log p_k|)``; the existing max-norm tolerances
  (1e-5, 1e-4, 1e-4) unchanged on top.
* J lives in a NaN-filled allocation with ``t_r > nc`` and ``t_b > n_rows t_r`` (any read outside a row's nc columns poisons the
  result), and also in the two contiguous layouts; every output is a NaN / sentinel-filled view between guard bands.
* Samples 0 and B - 1 carry the same J scaled by 2^3: their jtj agree bit for bit up to 2^6, their log-dets differ by d log 64.

Rank: with n_rows < d the Gram matrix is singular and the factorisation's verdict is rounding noise (the first n_rows pivots of a
rank-deficient Gram matrix may themselves be small), so those cases hold Gram, L1 terms, guards and the scale pair -- including
equal ``info`` -- and only the consistency of info / logdet / fail[0]; ``info == 0`` and the log-det bounds are asserted wherever
n_rows >= d, which every family has (n_rows = 160 was added to the two wide classes for that).  The cotangent form of the backward
kernel inverts G, so it runs where n_rows >= d; the explicit-matrix form runs at every row count.
"""
import ctypes as C
import math

import pytest
import torch

import _gram_head as H

pytestmark = pytest.mark.gpu

LAYOUTS = ("guarded", "panel", "fmajor")


@pytest.fixture(scope="module")
def lib():
    from cmf_amd import _lib
    return _lib.load()


def _ptr(p):
    return None if p is None else C.c_void_p(p)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lg(x):
    return f"2^{math.log2(x):.2f}" if x > 0 else "0"


def launch_forward(lib, panel, d, want_family, out=None):
    """One cmf_gram_cholesky launch (no retries) on a DevicePanel; the family is asserted first."""
    got = lib.cmf_gram_cholesky_family(panel.N, panel.nc, panel.t_r)
    assert got == want_family == H.family(panel.N, panel.nc, panel.t_r), (H.family_name(got), H.family_name(want_family))
    out = out or H.HeadOutputs(panel.B, d)
    rc = lib.cmf_gram_cholesky(_ptr(panel.ptr), panel.t_b, panel.t_r, panel.N, panel.nc, d, panel.B,
                               *[_ptr(p) for p in out.pointers()], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out.check_guards()
    return out


def enqueue_retries(lib, out, d, eps0=1e-6):
    jtj, logdet, _, l1_diag, info, fail = out.pointers()
    for a in range(1, 6):
        rc = lib.cmf_cholesky_retry(_ptr(jtj), d, out.B, a, eps0, _ptr(logdet), _ptr(l1_diag), _ptr(info), _ptr(fail), _stream())
        assert rc == 0, rc
    torch.cuda.synchronize()
    out.check_guards()


class Reference:
    """float64 quantities of one batch, computed once and shared by the layouts."""

    def __init__(self, J, d):
        self.J, self.d, self.n = J, d, J.shape[1]
        self.G, self.A = H.gram64(J, d)
        self.off, self.diag = H.l1_terms(self.G)
        self.off_A, self.diag_A = H.l1_terms(self.A)
        self.full_rank = self.n >= d
        if self.full_rank:
            self.logdet = torch.linalg.slogdet(self.G)[1]
            self.ld_scale = H.logdet_scale(self.G, self.A)


def check_forward(r, ref, tag):
    """Per-element, per-sample and max-norm assertions on one launch's outputs; returns the ratios reached."""
    d, B = ref.d, ref.J.shape[0]
    jtj = r["jtj"]
    assert bool(torch.isfinite(jtj).all()), f"{tag}: jtj not finite (a read outside a row's nc columns, or an unwritten element)"
    rg = H.ratio(jtj - ref.G, ref.A)
    depth = H.l1_sum_depth(d) * 2.0 ** -24
    b_off = H.C_GRAM * ref.off_A + depth * (ref.off + H.C_GRAM * ref.off_A)
    b_diag = H.C_GRAM * ref.diag_A + depth * (ref.diag + H.C_GRAM * ref.diag_A)
    ro, rd = H.ratio(r["l1_off"] - ref.off, b_off), H.ratio(r["l1_diag"] - ref.diag, b_diag)
    mx = float((jtj.double() - ref.G).abs().max() / ref.G.abs().max())
    line = f"GRAM_HEAD {tag}: Gram {_lg(rg)} of A (C {_lg(H.C_GRAM)}) max-norm {mx:.2e}  l1_off {ro:.3f} l1_diag {rd:.3f} of bound"
    info, ld = r["info"], r["logdet"]
    rl = None
    if ref.full_rank:
        rl = H.ratio(torch.nan_to_num(ld.double() - ref.logdet, nan=math.inf), ref.ld_scale)
        mxl = float((ld.double() - ref.logdet).abs().max() / ref.logdet.abs().max().clamp_min(1e-30))
        line += f"  log-det {_lg(rl)} (C {_lg(H.C_LOGDET)}) max-norm {mxl:.2e}"
    print(line)
    assert rg <= H.C_GRAM, f"{tag}: Gram element {rg / H.C_GRAM:.2f} x the bound"
    assert ro <= 1 and rd <= 1, f"{tag}: L1 terms {ro:.2f} / {rd:.2f} x their bounds"
    assert mx < 1e-5
    assert float((r["l1_off"].double() - ref.off).abs().max()) <= 1e-5 * float(ref.off.abs().max())
    assert float((r["l1_diag"].double() - ref.diag).abs().max()) <= 1e-5 * float(ref.diag.abs().max())
    # the scale pair: bit-identical up to 2^(2 SCALE_EXP)
    assert torch.equal(jtj[B - 1], jtj[0] * 4.0 ** H.SCALE_EXP), f"{tag}: samples 0 and B - 1 disagree beyond their scale"
    assert int(info[0]) == int(info[B - 1])
    fail = r["fail"].tolist()
    assert fail[1:] == [0] * 7 and fail[0] == int(bool((info != 0).any())), (fail, info.tolist())
    assert bool(((info >= 0) & (info <= d)).all())
    assert torch.equal(torch.isnan(ld), info != 0), f"{tag}: logdet must be NaN exactly where info != 0"
    if ref.full_rank:
        assert info.tolist() == [0] * B and fail[0] == 0, (info.tolist(), fail)
        assert rl <= H.C_LOGDET, f"{tag}: log-det {rl / H.C_LOGDET:.2f} x the bound"
        assert mxl < 1e-4, mxl                  # (sample B - 1 has log det >= d log 64 - |log det J_0|: the max-norm is never void)
        shift = float(ld[B - 1] - ld[0]) - d * 2 * H.SCALE_EXP * math.log(2.0)
        assert abs(shift) <= H.C_LOGDET * float(ref.ld_scale[0] + ref.ld_scale[B - 1]), shift
    return rg, rl


@pytest.mark.parametrize("fam,d,n_rows", H.FORWARD_CASES, ids=[f"{f}-d{d}-n{n}" for f, d, n in H.FORWARD_CASES])
def test_forward_per_element(lib, fam, d, n_rows):
    J = H.build_batch(n_rows, d, H.case_cond(d, n_rows), H.case_seed(d, n_rows))
    ref = Reference(J, d)
    first = None
    for layout in LAYOUTS:
        panel = H.DevicePanel(J, layout)
        out = launch_forward(lib, panel, d, H.expected_family(fam, d))
        assert panel.untouched_outside()
        r = out.read()
        check_forward(r, ref, f"{H.family_name(H.expected_family(fam, d))} d {d} nc {panel.nc} n_rows {n_rows} {layout}")
        if first is None:
            first = r
        else:                                   # the strides change addresses only: identical bits in every layout
            for k in ("jtj", "l1_off", "l1_diag", "info"):
                assert torch.equal(first[k], r[k]), (layout, k)
            assert torch.equal(torch.nan_to_num(first["logdet"], nan=-1.0), torch.nan_to_num(r["logdet"], nan=-1.0))


@pytest.mark.parametrize("nc,d", [(32, 17), (64, 61), (128, 128)])
def test_forward_big_span_runs_the_staged_kernel(lib, nc, d):
    """A panel spanning 2.1 GiB from 17 rows (t_r = 2^25 floats; row 16 starts exactly 2^31 bytes in): the ring kernels' 32-bit
    byte offsets cannot address it, the family is staged<nc / 16> (asserted BEFORE the launch), and the result is held to the
    same bounds.  Three samples sit side by side in each row (t_b = 256); NaN on both sides of every row's 3 x 256 floats."""
    n_rows, t_r, t_b, B = 17, 2 ** 25, 256, 3
    assert H.ceil16(d) == nc
    gen = torch.Generator().manual_seed(H.case_seed(d, n_rows, 5))
    J = torch.zeros(B, n_rows, nc)
    J[0, :, :d] = H.build_J(n_rows, d, 1e2, gen).float()
    J[1, :, :d] = H.build_J(n_rows, d, 1e2, gen).float()
    J[2] = J[0] * 2.0 ** H.SCALE_EXP
    assert 4 * n_rows * t_r > 2 ** 31 and 4 * (n_rows - 1) * t_r >= 2 ** 31
    want = nc // 16
    assert lib.cmf_gram_cholesky_family(n_rows, nc, t_r) == want == H.family(n_rows, nc, t_r)
    raw = torch.empty(H.PAD + (n_rows - 1) * t_r + B * t_b + H.PAD, device="cuda")
    for r in range(n_rows):
        raw[r * t_r:r * t_r + H.PAD + B * t_b + H.PAD] = float("nan")
    index = (H.PAD + torch.arange(B)[:, None, None] * t_b + torch.arange(n_rows)[None, :, None] * t_r
             + torch.arange(nc)[None, None, :]).reshape(-1).cuda()
    raw[index] = J.reshape(-1).cuda()
    ptr = raw.data_ptr() + 4 * H.PAD
    assert ptr % 16 == 0
    out = H.HeadOutputs(B, d)
    rc = lib.cmf_gram_cholesky(_ptr(ptr), t_b, t_r, n_rows, nc, d, B, *[_ptr(p) for p in out.pointers()], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out.check_guards()
    check_forward(out.read(), Reference(J, d), f"staged<{want}> d {d} nc {nc} n_rows {n_rows} span 2.1 GiB")


# ---------------------------------------------------------------------------------------------------------------------------
BACKWARD_CASES = [(d, n) for d in H.BACKWARD_D for n in H.BACKWARD_ROWS]
SELECTIONS = [(a, o, c) for a in (1, 0) for o in (1, 0) for c in (1, 0)]


def _check_cotangent(dt, want, scale, c, tag, d):
    got = dt.dense()
    assert dt.untouched_outside(), f"{tag}: a store outside rows 0 .. n_rows - 1, columns 0 .. nc - 1"
    assert bool(torch.isfinite(got).all()), f"{tag}: an element of the cotangent was not written"
    if d < got.shape[2]:
        assert float(got[:, :, d:].abs().max()) == 0.0, f"{tag}: padding columns must be exactly 0"
    r = H.ratio(got[:, :, :d] - want, scale)
    mx = float((got[:, :, :d].double() - want).abs().max() / want.abs().max().clamp_min(1e-300))
    print(f"GRAM_HEAD {tag}: dJ {_lg(r)} of |J||M| (C {_lg(c)}) max-norm {mx:.2e}")
    assert r <= c, f"{tag}: {r / c:.2f} x the bound"
    assert mx < 1e-4
    return r


@pytest.mark.parametrize("d,n_rows", BACKWARD_CASES, ids=[f"d{d}-n{n}" for d, n in BACKWARD_CASES])
def test_backward_per_element(lib, d, n_rows):
    """cmf_gram_backward_matrix with a non-symmetric M at every row count, and cmf_gram_backward with every on / off combination of
    the three cotangents where J has full column rank, against float64 autograd; dt has strides of its own, is NaN-filled, and
    nothing outside its n_rows x nc payload may change."""
    nc, B = H.ceil16(d), 4
    J = H.build_batch(n_rows, d, H.BWD_COND, H.case_seed(d, n_rows, 1))
    gen = torch.Generator().manual_seed(d + n_rows)
    M = torch.randn(B, d, d, generator=gen)
    g = [torch.randn(B, generator=gen) for _ in range(3)]
    Jd = J[:, :, :d].double()
    panel = H.DevicePanel(J, "guarded")
    tag = f"backward d {d} nc {nc} n_rows {n_rows}"

    Md = M.cuda()
    dt = H.DevicePanel(torch.full((B, n_rows, nc), float("nan")), "guarded2")
    rc = lib.cmf_gram_backward_matrix(_ptr(panel.ptr), panel.t_b, panel.t_r, n_rows, nc, d, B, _ptr(Md.data_ptr()), _ptr(dt.ptr),
                                      dt.t_b, dt.t_r, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    S = M.double() + M.double().transpose(1, 2)
    _check_cotangent(dt, Jd @ S, Jd.abs() @ S.abs(), H.C_BWD_MATRIX, tag + " matrix", d)
    if n_rows < d:
        return

    out = launch_forward(lib, panel, d, lib.cmf_gram_cholesky_family(n_rows, nc, panel.t_r))
    assert out.read()["info"].tolist() == [0] * B
    G, _ = H.gram64(J, d)
    terms = H.backward_reference(J, d)                      # float64 autograd, one unit term at a time
    gd_dev = [x.cuda() for x in g]
    for sel in SELECTIONS:
        if sel == (0, 0, 0):
            continue
        w = [x.double() * s for x, s in zip(g, sel)]
        want = sum(wi[:, None, None] * t for wi, t in zip(w, terms))
        scale = Jd.abs() @ H.backward_M_abs(G, *w)
        dt = H.DevicePanel(torch.full((B, n_rows, nc), float("nan")), "guarded2" if sel[0] else "fmajor")
        args = [_ptr(x.data_ptr()) if s else None for x, s in zip(gd_dev, sel)]
        rc = lib.cmf_gram_backward(_ptr(panel.ptr), panel.t_b, panel.t_r, n_rows, nc, d, B, _ptr(out.jtj.t.data_ptr()), *args,
                                   _ptr(dt.ptr), dt.t_b, dt.t_r, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        _check_cotangent(dt, want, scale, H.C_BWD, f"{tag} cotangents {sel}", d)
    out.check_guards()


# ---------------------------------------------------------------------------------------------------------------------------
def _bits(r):
    return {k: v.clone().view(torch.int32) for k, v in r.items()}


@pytest.mark.parametrize("fam,d,n_rows,j", H.FAILURE_CASES, ids=[f"{f}-d{d}-n{n}-j{j}" for f, d, n, j in H.FAILURE_CASES])
def test_exact_zero_pivot_and_the_retry_chain(lib, fam, d, n_rows, j):
    """Sample 1 has columns j - 1 and j equal: rows j - 1 and j of its Gram matrix go through bit-identical operations, the IEEE
    division gives a factor of exactly 1 and the pivot at column j is an exact zero: info == j + 1 there and 0 elsewhere, its
    logdet NaN, fail[0] == 1.  The enqueued retries 1 ... 5 then take as many attempts as the jitter loop on the kernel's own float32
    jtj (the same count in float32 and float64), move EVERY sample's diagonal by exactly the float32 jitters, leave the
    off-diagonals bit-identical, refresh l1_diag, and the regular samples' log-dets match float64 slogdet of the jittered matrices."""
    B = 4
    J = H.build_failure_batch(n_rows, d, j)
    panel = H.DevicePanel(J, "guarded")
    out = launch_forward(lib, panel, d, H.expected_family(fam, d))
    r0 = out.read()
    want_info = [j + 1 if b == H.FAILURE_SAMPLE else 0 for b in range(B)]
    assert r0["info"].tolist() == want_info, r0["info"].tolist()
    assert r0["fail"].tolist() == [1] + [0] * 7
    assert torch.equal(torch.isnan(r0["logdet"]), torch.tensor(want_info) != 0)
    G0 = r0["jtj"]
    assert torch.equal(G0[H.FAILURE_SAMPLE, j], G0[H.FAILURE_SAMPLE, j - 1])
    G64, A = H.gram64(J, d)
    assert H.ratio(G0 - G64, A) <= H.C_GRAM

    _, _, a32 = H.jitter_loop(G0)
    _, want_jtj, a64 = H.jitter_loop(G0.double())
    assert a32 == a64 == 2
    enqueue_retries(lib, out, d)
    r1 = out.read()
    attempts = 1 + sum(1 for f in r1["fail"].tolist()[:6] if f)
    assert attempts == a32 and r1["fail"].tolist() == [1] + [0] * 7, r1["fail"].tolist()
    assert r1["info"].tolist() == [0] * B
    diag0, diag1 = torch.diagonal(G0, dim1=1, dim2=2), torch.diagonal(r1["jtj"], dim1=1, dim2=2)
    moved = diag0.clone()
    for eps in H.jitters(attempts):
        moved = moved + eps
    assert torch.equal(diag1, moved), "every sample's diagonal moves by exactly the float32 jitters"
    eye = torch.eye(d, dtype=torch.bool)
    assert torch.equal(r1["jtj"][:, ~eye], G0[:, ~eye]), "off-diagonals must be bit-identical"
    assert torch.equal(r1["l1_off"], r0["l1_off"])
    dsum = diag1.double().abs().sum(1)
    assert float((r1["l1_diag"].double() - dsum).abs().max()) <= H.l1_sum_depth(d) * 2.0 ** -24 * float(dsum.max())
    Gj = r1["jtj"].double()
    good = [b for b in range(B) if b != H.FAILURE_SAMPLE]
    ld64 = torch.linalg.slogdet(Gj)[1]
    rl = H.ratio((r1["logdet"].double() - ld64)[good], H.logdet_scale(Gj[good], A[good]))
    print(f"GRAM_HEAD {H.family_name(H.expected_family(fam, d))} d {d} n_rows {n_rows} zero pivot at {j}: attempts {attempts}  "
          f"log-det after the jitter {_lg(rl)} (C {_lg(H.C_LOGDET)})")
    assert rl <= H.C_LOGDET
    assert float((r1["logdet"].double() - ld64)[good].abs().max()) < 1e-4 * float(ld64[good].abs().max())
    assert bool(torch.isfinite(r1["logdet"]).all())


NOOP_CASES = [(f, d, n) for f, d, n, _ in H.FAILURE_CASES[::3]] + [("gram64", 17, 17), ("gram64", 48, 129), ("gram64", 64, 257)]


@pytest.mark.parametrize("fam,d,n_rows", NOOP_CASES, ids=[f"{f}-d{d}-n{n}" for f, d, n in NOOP_CASES])
def test_retries_are_no_ops_without_a_failure(lib, fam, d, n_rows):
    J = H.build_failure_batch(n_rows, d, 1, singular=False)
    out = launch_forward(lib, H.DevicePanel(J, "guarded"), d, H.expected_family(fam, d))
    r0 = out.read()
    assert r0["info"].tolist() == [0] * 4 and r0["fail"].tolist() == [0] * 8
    assert H.jitter_loop(r0["jtj"])[2] == 1
    enqueue_retries(lib, out, d)
    r1 = out.read()
    b0, b1 = _bits(r0), _bits(r1)
    for k in b0:
        assert torch.equal(b0[k], b1[k]), f"{k} changed although no attempt had failed"
