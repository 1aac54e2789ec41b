"""The leverage kernel on the GPU (csrc/leverage.hip), through ``engine.tangent_leverage`` and the C entry point: against
the numpy.longdouble reference on the same float32 inputs within the bounds tests/test_uncertainty_host.py derives from the
emulation, its output contract -- a symmetric cov, no negative lev, stats, the cov-only mode's bits --, guarded buffers, isolation,
determinism and refusals.  Needs an MI355X: run with ``-m gpu``.

Bounds, per sample (u = 2^-53, kappa_s the condition number of the unit-diagonal scaling of the normal matrix):
    ||G cov - I||_max <= C_COV d u || |G| |cov| ||_max
    |lev_i - lev_ref,i| <= C_LEV d u kappa_s lev_ref,i
    |stats[0] - sum_i lev_i| <= (D + 2) u sum_i lev_i,   stats[1] == max_i lev_i
The padding columns d .. nc - 1 of every Jacobian stack are filled with NaN."""
import math

import numpy as np
import pytest
import torch

import _gn_step_emulation as GN
import _leverage_emulation as LE
from test_gpu_projection import guarded, guards_intact, same_bits, stack

pytestmark = pytest.mark.gpu

NAN = float("nan")
LAYOUTS = ["panel", "fmajor"]
U = LE.U


def run(J, G, layout="panel"):
    """``engine.tangent_leverage`` in both modes on CPU inputs -> numpy (cov, lev, stats, info, cov of rows=False, its info)."""
    from cmf_amd import engine as E
    T, Gc = stack(J, layout), torch.as_tensor(G).cuda()
    keep = Gc.clone()
    r, c = E.tangent_leverage(T, Gc), E.tangent_leverage(T, Gc, rows=False)
    torch.cuda.synchronize()
    B, D, d = J.shape
    assert same_bits(Gc.cpu().numpy(), keep.cpu().numpy())           # gram is never written
    assert r.cov.shape == (B, d, d) and r.lev.shape == (B, D) and r.stats.shape == (B, 2) and r.info.shape == (B,)
    assert r.cov.dtype == r.lev.dtype == r.stats.dtype == torch.float64 and r.info.dtype == torch.int32
    assert c.lev is None and c.stats is None
    return tuple(v.cpu().numpy() for v in (r.cov, r.lev, r.stats, r.info, c.cov, c.info))


_REFERENCE = {}


def reference(D, d):
    """The inputs of one shape and their longdouble reference, computed once and shared (never modified)."""
    if (D, d) not in _REFERENCE:
        J, G = LE.inputs(D, d)
        _REFERENCE[D, d] = (J, G, [LE.reference(J[b], G[b]) for b in range(LE.BATCH)] if LE.well_posed(d, D) else None)
    return _REFERENCE[D, d]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", LE.WIDTHS)
@pytest.mark.parametrize("D", LE.ROWS)
def test_kernel_matches_the_reference(D, d, layout):
    J, G, ref = reference(D, d)
    cov, lev, stats, info, cov_only, info_only = run(J, G, layout)
    assert same_bits(cov_only, cov) and same_bits(info_only, info)   # rows=False: the full mode's bits
    if ref is None:                                                  # G of rank D < d: a refused pivot and a completed
        assert set(info.tolist()) <= {0, 1}                          # factorisation are both legitimate
        for b in range(LE.BATCH):
            assert info[b] == 0 or (np.isnan(cov[b]).all() and np.isnan(lev[b]).all() and np.isnan(stats[b]).all())
        return
    assert (info == 0).all()
    worst_c = worst_l = 0.0
    for b in range(LE.BATCH):
        cov_ref, lev_ref, _, _ = ref[b]
        rc, rl = LE.cov_ratio(G[b], cov[b]), LE.lev_ratio(G[b], lev[b], lev_ref)
        worst_c, worst_l = max(worst_c, rc), max(worst_l, rl)
        assert rc <= LE.C_COV and rl <= LE.C_LEV, f"sample {b}: cov {rc}, lev {rl}"
        assert np.array_equal(cov[b], cov[b].T)                      # symmetric bit for bit
        assert not np.signbit(lev[b]).any()                          # a sum of squares over positive pivots: never negative or -0.0
        total = lev[b].sum()
        assert abs(stats[b, 0] - total) <= (D + 2) * U * total and stats[b, 1] == lev[b].max()
        # G is float32(J^T J) of this J: the leverages sum to d
        assert abs(total - d) <= LE.trace_bound(J[b], G[b], cov_ref, lev_ref), f"sample {b}"
    print(f"D={D} d={d} {layout}: worst cov ratio 2^{math.log2(max(worst_c, 1e-300)):.2f} (bound {LE.C_COV:g}), worst lev ratio "
          f"2^{math.log2(max(worst_l, 1e-300)):.2f} (bound {LE.C_LEV:g})")
    assert torch.equal(torch.as_tensor(cov), torch.as_tensor(cov).transpose(1, 2))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_normal_matrix_need_not_be_the_gram_matrix_of_t(layout):
    """gram = K^T K of another stack of 40 rows (the recover case): cov and lev follow gram, not J^T J."""
    D, d = 64, 17
    J, _ = LE.inputs(D, d, seed=4)
    _, GK = LE.inputs(40, d, seed=5)
    cov, lev, stats, info, _, _ = run(J, GK, layout)
    assert (info == 0).all()
    for b in range(LE.BATCH):
        cov_ref, lev_ref, _, _ = LE.reference(J[b], GK[b])
        assert LE.cov_ratio(GK[b], cov[b]) <= LE.C_COV and LE.lev_ratio(GK[b], lev[b], lev_ref) <= LE.C_LEV


@pytest.mark.parametrize("B,D,d,layout", [(3, 64, 17, "panel"), (2, 784, 64, "fmajor"), (3, 5, 100, "panel"), (2, 64, 128, "fmajor")])
def test_outputs_stay_inside_their_buffers(B, D, d, layout):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    J, G = LE.inputs(D, d, B=B, seed=2)
    if D < d:                                                        # a well-posed normal matrix all the same: J^T J + diag
        G = (G + np.eye(d, dtype=np.float32) * np.float32(1e4)).astype(np.float32)
    T, Gc = stack(J, layout), torch.as_tensor(G).cuda()
    bufs = {"cov": guarded((B, d, d), torch.float64), "lev": guarded((B, D), torch.float64), "stats": guarded((B, 2), torch.float64),
            "info": guarded((B,), torch.int32), "cov_c": guarded((B, d, d), torch.float64), "info_c": guarded((B,), torch.int32)}
    p = lambda name: E._p(bufs[name][1])
    lib = _lib.load()
    _lib.check(lib.cmf_tangent_leverage(E._p(T.data), T.t_b, T.t_r, D, T.nc, d, B, E._p(Gc), p("cov"), p("lev"), p("stats"), p("info"),
                                        E._stream()), "cmf_tangent_leverage")
    _lib.check(lib.cmf_tangent_leverage(None, 0, 0, 0, 0, d, B, E._p(Gc), p("cov_c"), None, None, p("info_c"), E._stream()),
               "cmf_tangent_leverage")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    cov, lev, stats, info, cov_only, info_only = run(J, G, layout)
    got = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    assert (info == 0).all() and not np.isnan(lev).any() and not np.isnan(cov).any()      # every element is written
    assert same_bits(got["cov"], cov) and same_bits(got["lev"], lev) and same_bits(got["stats"], stats) and same_bits(got["info"], info)
    assert same_bits(got["cov_c"], cov) and same_bits(got["info_c"], info)


@pytest.mark.parametrize("D,d,layout", [(64, 17, "panel"), (784, 100, "panel"), (64, 17, "fmajor"), (70, 128, "fmajor")])
def test_position_independence_and_repeatability(D, d, layout):
    J, G = LE.inputs(D, d, seed=3)
    if D < d:
        G = (G + np.eye(d, dtype=np.float32) * np.float32(1e4)).astype(np.float32)
    where = [0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 2]
    base = run(J, G, layout)
    batch = run(J[where], G[where], layout)
    again = run(J[where], G[where], layout)
    assert (base[3] == 0).all()
    for a, b, c in zip(base, batch, again):
        assert same_bits(a[where], b) and same_bits(b, c)
    for b in range(3):
        for a, c in zip(run(J[b:b + 1], G[b:b + 1], layout), base):
            assert same_bits(a[0], c[b]), f"sample {b}"
    # the upper triangle of gram is never read
    upper = np.triu(np.ones((d, d), dtype=bool), 1)
    for a, b in zip(base, run(J, np.where(upper, np.float32(NAN), G), layout)):
        assert same_bits(a, b)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_failures_are_reported_and_confined(layout):
    D, d = 64, 5
    J, G = LE.inputs(D, d, B=6, seed=1)
    clean = run(J, G, layout)
    assert (clean[3] == 0).all()
    J[1, :, 3] = J[1, :, 1]                                          # a duplicate column: the pivot cancels exactly
    G[1] = GN.gram_by_dots(J[1])
    J[2, 40, 4] = NAN                                                # in the second slab of rows
    G[3, 4, 2] = NAN
    J[4, 3, 1] = np.inf
    G[4] = G[1]                                                      # a refused pivot AND a non-finite row: 2 wins
    cov, lev, stats, info, cov_only, info_only = run(J, G, layout)
    assert info.tolist() == [0, 1, 2, 2, 2, 0]
    assert info_only.tolist() == [0, 1, 0, 2, 1, 0]                  # the cov-only mode does not look at J
    for b in (1, 2, 3, 4):
        assert np.isnan(cov[b]).all() and np.isnan(lev[b]).all() and np.isnan(stats[b]).all()
    for b in (0, 5):                                                 # the neighbours are untouched, bit for bit
        for got, want in zip((cov, lev, stats, cov_only), (clean[0], clean[1], clean[2], clean[4])):
            assert same_bits(got[b], want[b])
    assert same_bits(cov_only[2], clean[4][2]) and np.isnan(cov_only[[1, 3, 4]]).all()


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    B, D, d = 2, 8, 3
    J, G = LE.inputs(D, d, B=B)
    T, Gc = stack(J, "panel"), torch.as_tensor(G).cuda()
    cov = torch.zeros(B * d * d + 1, dtype=torch.float64, device="cuda")
    lev = torch.zeros(B * D + 1, dtype=torch.float64, device="cuda")
    stats = torch.zeros(2 * B + 1, dtype=torch.float64, device="cuda")
    info = torch.full((B + 1,), -5, dtype=torch.int32, device="cuda")
    odd = lambda t: t.data_ptr() + 4                               # a float64 pointer that is only 4-byte aligned
    ok = [E._p(T.data), T.t_b, T.t_r, D, T.nc, d, B, E._p(Gc), E._p(cov), E._p(lev), E._p(stats), E._p(info)]
    assert lib.cmf_tangent_leverage(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert info[:B].tolist() == [0, 0] and float(lev.sum()) > 0
    for t in (cov, lev, stats):
        t.zero_()
    info.fill_(-5)
    bad = [(1, T.t_b + 2), (2, T.t_r + 2), (2, 8), (1, 8), (3, 0), (4, 24), (4, 0), (5, 0), (5, 129), (5, 17), (6, 0), (7, None),
           (8, None), (9, None), (10, None), (11, None), (0, E._p(T.data[1:])), (8, odd(cov)), (9, odd(lev)), (10, odd(stats)),
           (7, Gc.data_ptr() + 2), (11, info.data_ptr() + 2)]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_tangent_leverage(*args, E._stream()) == -1, (i, value)
    # cov-only mode: gram, cov, info, d and B are still required
    only = [None, 0, 0, 0, 0, d, B, E._p(Gc), E._p(cov), None, None, E._p(info)]
    for i, value in ((5, 0), (5, 129), (6, 0), (7, None), (8, None), (11, None), (8, odd(cov))):
        args = list(only)
        args[i] = value
        assert lib.cmf_tangent_leverage(*args, E._stream()) == -1, (i, value)
    torch.cuda.synchronize()
    assert float(cov.abs().sum()) == 0.0 and float(lev.abs().sum()) == 0.0 and float(stats.abs().sum()) == 0.0
    assert bool((info == -5).all())


def test_engine_refusals():
    from cmf_amd import engine as E
    J, G = LE.inputs(8, 3, B=2)
    T, Gc = stack(J, "panel"), torch.as_tensor(G).cuda()
    with pytest.raises(ValueError, match="engine.Tangent"):
        E.tangent_leverage(T.data, Gc)
    with pytest.raises(ValueError, match="float32"):
        E.tangent_leverage(T, Gc.double())
    with pytest.raises(ValueError, match="not contiguous"):
        E.tangent_leverage(T, Gc.transpose(1, 2))
    with pytest.raises(ValueError, match=r"contiguous \(B, d, d\)"):
        E.tangent_leverage(T, Gc[:, :, :2].contiguous())
    with pytest.raises(ValueError, match="GPU"):
        E.tangent_leverage(T, Gc.cpu())
    with pytest.raises(ValueError, match="the leverage kernel supports 1 <= d <= 128"):
        E.tangent_leverage(E.Tangent(2, 8, 144, "panel", "cuda"), torch.zeros(2, 129, 129, device="cuda"))
    with pytest.raises(ValueError, match="must hold d = 3 <= nc columns"):
        E.tangent_leverage(T, Gc[:1].contiguous())
    with pytest.raises(ValueError, match="must hold d = 17 <= nc columns"):
        E.tangent_leverage(T, torch.zeros(2, 17, 17, device="cuda"))
    with pytest.raises(ValueError, match="nc % 16 == 0"):
        E.tangent_leverage(E.Tangent(2, 8, 8, "panel", "cuda"), Gc)
    # B == 0: empties, no launch
    r = E.tangent_leverage(E.Tangent(0, 8, 16, "panel", "cuda"), Gc[:0])
    assert r.cov.shape == (0, 3, 3) and r.lev.shape == (0, 8) and r.stats.shape == (0, 2) and r.info.shape == (0,)
    r = E.tangent_leverage(E.Tangent(0, 8, 16, "panel", "cuda"), Gc[:0], rows=False)
    assert r.cov.shape == (0, 3, 3) and r.lev is None and r.stats is None


def test_kernel_timer_entry():
    from cmf_amd import engine as E
    J, G = LE.inputs(8, 3, B=2)
    T, Gc = stack(J, "panel"), torch.as_tensor(G).cuda()
    with E.timing(lambda name: True) as timer:
        E.tangent_leverage(T, Gc)
    full = timer.by_name()
    with E.timing(lambda name: True) as timer:
        E.tangent_leverage(T, Gc, rows=False)
    only = timer.by_name()
    assert set(full) == set(only) == {"tangent_leverage"}
    assert all(n == 1 and ms >= 0 and flops > 0 and nbytes > 0 for n, ms, flops, nbytes in (full["tangent_leverage"], only["tangent_leverage"]))
    assert only["tangent_leverage"][2] < full["tangent_leverage"][2] and only["tangent_leverage"][3] < full["tangent_leverage"][3]
