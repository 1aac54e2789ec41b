"""Host-side checks behind tests/test_gpu_gram_head.py (no GPU needed): the dispatch predicate of ``cmf_gram_cholesky`` against its
exact-integer restatement over a grid that brackets every boundary, the 32-bit offset arithmetic of the two ring kernels walked
loop by loop, the bound constants of tests/_gram_head.py against the float32 CPU emulations on the GPU tests' own inputs (a factor
of four below each constant) and against the same emulations with planted defects (above each constant), and the jitter loop."""
import math

import pytest
import torch

import _gram_head as H


@pytest.fixture(scope="module")
def lib():
    from cmf_amd.build import build
    from cmf_amd import _lib
    build(verbose=False)
    return _lib.load()


def _t_r_grid(nc, n_rows):
    out = {nc, nc + 4, nc + 12, 4 * nc}
    for k in range(8, 31):
        out |= {2 ** k - 4, 2 ** k, 2 ** k + 4}
    # the stride at which ring_top crosses RING_LIMIT, bracketed (ring_top is affine in t_r)
    if nc in (32, 48, 64, 128):
        slope = (H.ring_top(n_rows, nc, 8) - H.ring_top(n_rows, nc, 4)) // 4
        star = (H.RING_LIMIT - H.ring_top(n_rows, nc, 0)) // slope // 4 * 4
        out |= {star + 4 * k for k in range(-3, 4)}
        # ... and where the descriptor range alone (the guard this predicate replaces) crossed its limit
        old = H.RING_LIMIT // (4 * n_rows) // 4 * 4
        out |= {old - 4, old, old + 4}
    return sorted(t for t in out if nc <= t <= 2 ** 30)


N_ROWS_GRID = sorted({1, 2, 3, 4, 5, 16, 17, 31, 32, 33, 100, 127, 128, 129, 132, 257, 784, 3072}
                     | {2 ** k + e for k in range(9, 23) for e in (-1, 0, 1) if 2 ** k + e <= 2 ** 22})


def test_family_matches_its_restatement_and_ring_offsets_fit_32_bits(lib):
    """cmf_gram_cholesky_family == tests/_gram_head.family for nc 16 ... 144, n_rows 1 ... 2^22, t_r nc ... 2^30, with the strides
    around every point where a ring kernel's largest offset crosses the limit; and wherever the C function answers with a ring
    kernel, the largest byte offset that kernel forms (overshoot of the prefetch ring included) is below 2^31."""
    seen = set()
    for nc in range(16, 145, 16):
        for n_rows in N_ROWS_GRID:
            for t_r in _t_r_grid(nc, n_rows):
                got = lib.cmf_gram_cholesky_family(n_rows, nc, t_r)
                assert got == H.family(n_rows, nc, t_r), (n_rows, nc, t_r, got)
                seen.add((nc, got))
                if got in (H.RING64, H.DIRECT128):
                    assert H.ring_top(n_rows, nc, t_r) < 2 ** 31
                    if n_rows <= 4096:
                        top, panel = H.ring_offsets_walk(n_rows, nc, t_r)
                        assert top < 2 ** 31 and panel < 2 ** 31, (n_rows, nc, t_r, top)
                elif nc in (32, 48, 64, 128):
                    assert got == nc // 16 and H.ring_top(n_rows, nc, t_r) >= H.RING_LIMIT
    # every class is reached on both sides of its guard
    for nc in (32, 48, 64):
        assert (nc, H.RING64) in seen and (nc, nc // 16) in seen
    assert (128, H.DIRECT128) in seen and (128, 8) in seen and (144, H.WIDE) in seen
    assert {(nc, nc // 16) for nc in (16, 80, 96, 112)} <= seen


def test_family_edges(lib):
    f = lib.cmf_gram_cholesky_family
    for bad in [(0, 64, 64), (-1, 64, 64), (10, 0, 64), (10, 24, 64), (10, 528, 528), (10, 64, 60), (10, 64, 66), (10, -16, 64)]:
        assert f(*bad) == H.INVALID == H.family(*bad), bad
    assert f(10, 512, 512) == H.WIDE and f(10, 144, 144) == H.WIDE
    # the benchmarked and documented shapes keep their kernels
    assert f(784, 64, 64) == H.RING64 and f(3072, 128, 128) == H.DIRECT128 and f(784, 16, 16) == 1
    assert f(784, 64, 512 * 64) == H.RING64 and f(784, 48, 4096 * 48) == H.RING64          # feature-major, large batches
    # the two defects the old dispatcher had: nc 128 unguarded; nc <= 64 guarded by the descriptor range alone
    assert f(17, 128, 2 ** 25) == 8 and f(2 ** 22, 128, 128) == 8                          # 2.1 GiB panels
    n_rows, t_r = 17, 2 ** 24                                                              # panel 1.06 GiB < limit, ring end 2.1 GiB
    assert 4 * n_rows * t_r < H.RING_LIMIT <= H.ring_top(n_rows, 64, t_r) and f(n_rows, 64, t_r) == 4
    assert f(17, 32, 2 ** 25) == 2 and f(17, 64, 2 ** 25) == 4


@pytest.mark.parametrize("nc", [32, 48, 64, 128])
def test_closed_form_of_the_ring_offsets_is_the_walk(nc):
    """``ring_top`` (what the predicate evaluates) against a literal walk of the kernels' load loops, wave by wave and lane by lane,
    for every row count 1 ... 600 and long panels: never below the walk (no load is under-counted), and above it by less than 12
    rows + 256 bytes (the closed form pairs wave 0's group count with wave 3's lane rows and ignores the lane mask of nc < 64);
    equal for the nc = 128 kernel, whose waves all walk the same groups."""
    for n_rows in list(range(1, 601)) + [4095, 4096, 4097, 65537]:
        for t_r in (nc, nc + 12, 4096):
            top, panel = H.ring_offsets_walk(n_rows, nc, t_r)
            closed = H.ring_top(n_rows, nc, t_r)
            assert panel <= top <= closed <= top + (0 if nc == 128 else 48 * t_r + 256), (n_rows, nc, t_r, top, closed)


def test_staged_kernel_lds_fits_at_every_width():
    """gram_chol_kernel<NT> for NT = 1 ... 8 (8: the new big-panel route of nc = 128): 32 x LDJ + NC x (NC + 1) floats within the
    160 KiB of a gfx950 workgroup."""
    for nt in range(1, 9):
        nc = 16 * nt
        ldj = nc + 16 if nc % 32 == 0 else nc
        assert (H.KC * ldj + nc * (nc + 1)) * 4 <= 160 * 1024
    assert H.KC * 144 + 128 * 129 == 21120


# ---------------------------------------------------------------------------------------------------------------------------
def _forward(fam, d, n):
    J = H.build_batch(n, d, H.case_cond(d, n), H.case_seed(d, n))
    G, A = H.gram64(J, d)
    return J, G, A, H.emulate_gram(J, d, 4 if fam == "gram64" else 1)


def test_forward_emulation_is_a_factor_of_four_inside_the_bounds():
    """Every forward input of the GPU test: the float32 emulation of the Gram accumulation (4-row groups, 4-plane sum for the
    nc <= 64 kernel) is within C_GRAM / 4 of float64 per element, its L1 terms within a quarter of their bound, and, where J has
    full column rank, the emulated elimination's log-det within C_LOGDET / 4 per sample and 1e-4 in the max-norm."""
    wg = wl = 0.0
    for fam, d, n in H.FORWARD_CASES:
        J, G, A, Ge = _forward(fam, d, n)
        assert torch.equal(Ge[-1], Ge[0] * 4.0 ** H.SCALE_EXP)                  # the power-of-two copy is exact in float32
        wg = max(wg, H.ratio(Ge - G, A))
        if n >= d:
            ld, info = H.emulate_elimination(Ge)
            assert int(info.max()) == 0
            ld64 = torch.linalg.slogdet(G)[1]
            wl = max(wl, H.ratio(ld - ld64, H.logdet_scale(G, A)))
            assert float((ld.double() - ld64).abs().max() / ld64.abs().max()) < 1e-4
    print(f"forward emulation: Gram 2^{math.log2(wg):.2f} of A (C_GRAM 2^{math.log2(H.C_GRAM):.0f}), "
          f"log-det 2^{math.log2(wl):.2f} (C_LOGDET 2^{math.log2(H.C_LOGDET):.0f})")
    assert 4 * wg <= H.C_GRAM and 4 * wl <= H.C_LOGDET


DEFECT_SHAPES = [("staged1", 16, 100), ("gram64", 33, 257), ("gram64", 64, 257), ("staged567", 80, 160), ("staged567", 112, 160),
                 ("direct128", 128, 160)]


def _defects(fam, d, n, J):
    """The four planted defects as Gram matrices of the emulation."""
    planes = 4 if fam == "gram64" else 1
    out = {}
    weakest = 1 if n > 1 else 0                                                  # a row of the smallest weight (0.5)
    Jd = J.clone()
    Jd[:, weakest] = 0
    out["row dropped"] = H.emulate_gram(Jd, d, planes)
    Jd = J.clone()
    Jd[:-1, n - 1] = J[1:, n - 1]
    Jd[-1, n - 1] = J[0, n - 1]
    out["last row of the neighbour"] = H.emulate_gram(Jd, d, planes)
    G = H.emulate_gram(J, d, planes)
    c1, c2 = H.swap_pair(d)
    Gs = G.clone()
    Gs[:, [c1, c2]] = G[:, [c2, c1]]                                             # J columns swapped on the A side only
    out["columns swapped on one side"] = Gs
    Gz = G.clone()
    it, jt = (d - 1) // 16, 0
    Gz[:, 16 * it:16 * it + 16, 16 * jt:16 * jt + 16] = 0
    out["tile left at zero"] = Gz
    return out


@pytest.mark.parametrize("fam,d,n", DEFECT_SHAPES)
def test_planted_forward_defects_leave_the_bounds(fam, d, n):
    """One J row (of the smallest weight) dropped; the last row taken from the neighbouring sample; two columns inside one
    16-tile swapped on one side; one off-diagonal tile of the grid (NT = 5 at d = 80) left at zero: each is outside C_GRAM per
    element and outside C_LOGDET per sample, at the largest row counts of the GPU test (where one row weighs least)."""
    J = H.build_batch(n, d, 1e2, H.case_seed(d, n, 3))
    G, A = H.gram64(J, d)
    ld64, scale = torch.linalg.slogdet(G)[1], H.logdet_scale(G, A)
    if d > 16:
        assert _defects(fam, d, n, J)["tile left at zero"][:, -1, 0].abs().max() == 0
    for name, Gd in _defects(fam, d, n, J).items():
        rg = H.ratio(Gd - G, A)
        assert rg > 4 * H.C_GRAM, (name, rg)
        ld, info = H.emulate_elimination(Gd)
        rl = H.ratio(torch.nan_to_num(ld.double() - ld64, nan=math.inf), scale)
        print(f"{fam} d {d} n {n} {name}: Gram 2^{math.log2(rg):.1f}, log-det 2^{math.log2(rl):.1f}")
        assert rl > 4 * H.C_LOGDET, (name, rl)


def _backward(d, n):
    J = H.build_batch(n, d, H.BWD_COND, H.case_seed(d, n, 1))
    gen = torch.Generator().manual_seed(d + n)
    M = torch.randn(4, d, d, generator=gen)
    g = [torch.randn(4, generator=gen) for _ in range(3)]
    return J, M, g


def test_backward_emulation_is_a_factor_of_four_inside_the_bounds():
    wb = wm = 0.0
    for d in H.BACKWARD_D:
        for n in H.BACKWARD_ROWS:
            J, M, (ga, go, gd) = _backward(d, n)
            Jd, S = J[:, :, :d].double(), M.double() + M.double().transpose(1, 2)
            wm = max(wm, H.ratio(J[:, :, :d] @ (M + M.transpose(1, 2)) - Jd @ S, Jd.abs() @ S.abs()))
            if n >= d:
                G, _ = H.gram64(J, d)
                got, _ = H.emulate_backward(J, d, H.emulate_gram(J, d, 1), ga, go, gd)
                M64 = H.backward_M(G, ga.double(), go.double(), gd.double())
                wb = max(wb, H.ratio(got - Jd @ M64, Jd.abs() @ H.backward_M_abs(G, ga.double(), go.double(), gd.double())))
                # the float64 autograd reference IS J M64
                terms = H.backward_reference(J, d)
                auto = sum(w.double()[:, None, None] * t for w, t in zip((ga, go, gd), terms))
                assert H.ratio(auto - Jd @ M64, Jd.abs() @ M64.abs()) < 1e-12
    print(f"backward emulation: 2^{math.log2(wb):.2f} (C_BWD 2^{math.log2(H.C_BWD):.0f}), matrix form 2^{math.log2(wm):.2f} "
          f"(C_BWD_MATRIX 2^{math.log2(H.C_BWD_MATRIX):.0f})")
    assert 4 * wb <= H.C_BWD and 4 * wm <= H.C_BWD_MATRIX


@pytest.mark.parametrize("d,n", [(20, 100), (80, 160), (100, 160), (128, 160)])
def test_planted_backward_defects_leave_the_bounds(d, n):
    """dJ = J M emulated in float32 with: one J row dropped, the last row read from the neighbouring sample, two columns of M
    inside one 16-tile swapped, a 4-column group of one row left at zero: all outside both constants."""
    J, M, (ga, go, gd) = _backward(d, n)
    Jd = J[:, :, :d].double()
    G, _ = H.gram64(J, d)
    M64 = H.backward_M(G, ga.double(), go.double(), gd.double())
    M32 = H.emulate_backward(J, d, H.emulate_gram(J, d, 1), ga, go, gd)[1]
    S32, S64 = M + M.transpose(1, 2), M.double() + M.double().transpose(1, 2)
    Mabs = H.backward_M_abs(G, ga.double(), go.double(), gd.double())
    for Mf, Md, Ma, c in ((M32, M64, Mabs, H.C_BWD), (S32, S64, S64.abs(), H.C_BWD_MATRIX)):
        want, scale = Jd @ Md, Jd.abs() @ Ma
        good = J[:, :, :d] @ Mf
        assert H.ratio(good - want, scale) <= c / 4
        bad = good.clone()
        bad[:, 1] = 0
        assert H.ratio(bad - want, scale) > 4 * c
        bad = good.clone()
        bad[:-1, n - 1] = good[1:, n - 1]
        assert H.ratio(bad - want, scale) > 4 * c
        c1, c2 = H.swap_pair(d)
        Ms = Mf.clone()
        Ms[:, [c1, c2]] = Mf[:, [c2, c1]]
        assert H.ratio(J[:, :, :d] @ Ms - want, scale) > 4 * c
        bad = good.clone()
        bad[:, n // 2, :4] = 0
        assert H.ratio(bad - want, scale) > 4 * c


@pytest.mark.parametrize("nc", [16, 32, 48, 64, 80, 96, 112, 128])
def test_backward_thread_map_covers_every_store_once(nc):
    """The product phase of gram_backward_kernel: thread (rg, q) = (tid / nq, tid % nq), nq = nc / 4, stores columns 4 q .. 4 q + 3
    of the slab rows rg, rg + rpp, ... behind ``rg < rpp``.  For every slab height each (row, q) is stored exactly once, the idle
    threads exist exactly at nq = 12, 20, 24, 28 (nc = 48, 80, 96, 112), and the mutant ``rg <= rpp`` lets them store rows rpp, 2 rpp, ...
    of the slab a second time -- rows the group rg = 0 also owns, from the same operands: the same set of addresses, no store
    outside the slab.  That mutant is therefore not observable in the output."""
    nq = nc // 4
    for nr in (1, 2, 9, 10, 11, 12, 13, 31, 32):
        plain, mutant = H.backward_store_map(nc, nr), H.backward_store_map(nc, nr, mutant=True)
        assert sorted(plain) == [(r, q) for r in range(nr) for q in range(nq)]
        assert set(mutant) == set(plain)
        idle = 256 - (256 // nq) * nq
        assert (idle > 0) == (nc in (48, 80, 96, 112))
        assert len(mutant) - len(plain) == idle * len(range(256 // nq, nr, 256 // nq))


def test_jitter_loop_counts_agree_in_float32_and_float64():
    """Failure inputs: the emulated float32 Gram matrix has bit-identical rows j - 1 and j, the pivot-only elimination meets an
    exact zero at column j (info = j + 1) in float32 and in float64, one jitter of 1e-6 repairs it in both precisions (2 attempts),
    and from the jittered matrix on LAPACK (the oracle's ``cholesky_logdet``) agrees with the restated loop.  Without the singular
    sample the loop takes one attempt and the oracle's own loop says the same."""
    from oracle import cmf_oracle as O
    for fam, d, n, j in H.FAILURE_CASES:
        J = H.build_failure_batch(n, d, j)
        G32 = H.emulate_gram(J, d, 1)
        assert torch.equal(G32[H.FAILURE_SAMPLE, j], G32[H.FAILURE_SAMPLE, j - 1])
        ld, info = H.emulate_elimination(G32)
        want_info = [j + 1 if b == H.FAILURE_SAMPLE else 0 for b in range(4)]
        assert info.tolist() == want_info and H.eliminate(G32.double())[1].tolist() == want_info
        ld32, out32, a32 = H.jitter_loop(G32)
        ld64, out64, a64 = H.jitter_loop(G32.double())
        assert a32 == a64 == 2, (fam, d, n, j, a32, a64)
        assert torch.equal(torch.diagonal(out32, dim1=1, dim2=2),
                           torch.diagonal(G32, dim1=1, dim2=2) + H.jitters(2)[0])
        ldo, _, ao = O.cholesky_logdet(out64)
        assert ao == 1 and float((ldo[:, 0] - ld64).abs().max()) < 1e-9 * d
        good = [b for b in range(4) if b != H.FAILURE_SAMPLE]
        assert float((ld32.double() - ld64)[good].abs().max()) < 1e-4 * float(ld64[good].abs().max())
        clean = H.emulate_gram(H.build_failure_batch(n, d, j, singular=False), d, 1)
        assert H.jitter_loop(clean)[2] == 1 and H.jitter_loop(clean.double())[2] == 1
        assert O.cholesky_logdet(clean)[2] == 1 and O.cholesky_logdet(clean.double())[2] == 1
    e = [float(x) for x in H.jitters(4)]
    assert len(e) == 3 and e[0] == float(torch.tensor(1e-6, dtype=torch.float32)) and 9.9e-5 < e[2] < 1.01e-4


def test_ratio_counts_zero_over_zero_as_zero():
    z = torch.zeros(2, dtype=torch.float64)
    assert H.ratio(z, z) == 0.0 and H.ratio(torch.tensor([1e-9, 0.0]), z) == math.inf
    assert H.ratio(torch.tensor([0.5]), torch.tensor([2.0])) == 0.25
