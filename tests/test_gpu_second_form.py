"""The second-form kernel on the GPU (csrc/second_form.hip) against extended-precision numpy on the same float32 inputs:
the bound forms of tests/_second_form_emulation.py (which tests/test_curvature_host.py holds the numpy emulation to), known answers
whose inputs are exact in float32, the failure codes, isolation, determinism and the refusals of the entry point and of
``engine.second_form``.  Needs an MI355X: run with ``-m gpu``.

The strict upper triangle of every matrix handed to the kernel is NaN, and so are the column slots >= m of the shifted stack and >= d of
the centre stack."""
import numpy as np
import pytest
import torch

import _second_form_emulation as SE
from test_gpu_projection import guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu

NAN = float("nan")
LAYOUTS = ["panel", "fmajor"]
NAMES = ("second_gram", "christoffel", "frame_metric", "stats", "info")


def stack(dense, nc, layout):
    """A CPU (B, D, n) float32 array as an ``engine.Tangent`` of nc column slots on the GPU whose padding columns are NaN."""
    from cmf_amd import engine as E
    B, D, n = dense.shape
    full = np.full((B, D, nc), np.float32(NAN), dtype=np.float32)
    full[:, :, :n] = dense
    return E.Tangent.from_dense(torch.as_tensor(full).cuda(), nc, layout)


def device_inputs(cs, layout):
    Jd, jtj, Sd, frame, step, nc = cs
    return (stack(Jd, nc, layout), torch.as_tensor(jtj).cuda(), stack(Sd, 16, layout), torch.as_tensor(frame).cuda(),
            torch.as_tensor(step).cuda())


def run(cs, layout="panel"):
    """``engine.second_form`` on a case of the emulation module -> numpy (second_gram, christoffel, frame_metric, stats, info)."""
    from cmf_amd import engine as E
    r = E.second_form(*device_inputs(cs, layout))
    torch.cuda.synchronize()
    return tuple(getattr(r, k).cpu().numpy() for k in NAMES)


@pytest.mark.parametrize("d", SE.WIDTHS)
def test_bounds_at_every_width(d):
    worst = {}
    for m in SE.FRAMES:
        if m > d:
            continue
        for D in SE.rows_of(d):
            for B in SE.BATCHES:
                cs = SE.case(B, d, m, D)
                exs = SE.exacts(cs)                                  # the extended-precision values once, for both layouts
                for layout in LAYOUTS:
                    got = run(cs, layout)
                    assert (got[4] == 0).all(), (m, D, B, layout)
                    assert got[0].shape == (B, m * (m + 1) // 2, m * (m + 1) // 2) and got[1].shape[1:] == (m * (m + 1) // 2, d)
                    assert same_bits(got[0], got[0].transpose(0, 2, 1)) and same_bits(got[2], got[2].transpose(0, 2, 1))
                    ratios = SE.worst_ratios(cs, got, exs)
                    for k, v in ratios.items():
                        worst[k] = max(worst.get(k, 0.0), v)
                    assert all(v <= 1.0 for v in ratios.values()), (m, D, B, layout, ratios)
                    if m > 1:
                        assert (got[3][:, 0] > 0).all() and (got[3][:, 1] > 0).all()      # the asymmetry sums are non-trivial
                    else:
                        assert (got[3][:, :2] == 0).all()
    print(f"d={d}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_both_layouts_give_the_same_bits(layout):
    for d, m, D in ((3, 2, 6), (17, 4, 20), (65, 3, 68), (128, 4, 178)):
        cs = SE.case(3, d, m, D)
        for a, b in zip(run(cs, layout), run(cs, "panel")):
            assert same_bits(a, b)


def test_quadratic_graphs():
    """Known answer (i): graphs of small-integer quadratic forms; every input and the central difference are exact."""
    rng = np.random.default_rng(11)
    for d, m, K in ((2, 2, 1), (3, 3, 2), (5, 4, 3), (17, 4, 2)):
        Q = rng.integers(-2, 3, (K, d, d)).astype(np.float64)
        Q = Q + Q.transpose(0, 2, 1)
        frame = rng.integers(-2, 3, (m, d)).astype(np.float64) + 3.0 * np.eye(m, d)
        cs, H = SE.quadratic_graph(Q, np.zeros(d), frame, 2.0 ** -3)
        got = run(cs)
        assert got[4][0] == 0
        # at z = 0 the tangent plane is the latent plane: H is normal, N = H H^T exactly up to the N bound
        assert SE.worst_ratios(cs, got)["N"] <= 1.0
        ex = SE.exact(cs[0][0], cs[1][0], cs[2], cs[3][0], cs[4][0])
        assert (ex["N"] == H @ H.T).all()                            # small integers over a power of two: the exact value is exact
        assert same_bits(got[3][0, 0], 0.0)                          # (iii): a symmetric stack has no asymmetry, exactly
    for k1, k2, z in ((1.0, 2.0, (0.5, -0.25)), (2.0, -1.0, (0.25, 0.5)), (1.0, 1.0, (0.0, 0.0))):
        Q = np.diag([k1, k2])[None]
        cs, _ = SE.quadratic_graph(Q, np.array(z), np.eye(2), 2.0 ** -3)
        N, _, g, st, info = (v[0] for v in run(cs))
        assert info == 0 and st[0] == 0.0
        K01 = (N[0, 2] - N[1, 1]) / (g[0, 0] * g[1, 1] - g[0, 1] ** 2)
        want = k1 * k2 / (1.0 + (k1 * z[0]) ** 2 + (k2 * z[1]) ** 2) ** 2
        assert abs(K01 - want) <= 1e-13 * abs(want), (K01, want)


@pytest.mark.parametrize("d,m,D", [(2, 2, 5), (5, 3, 9), (17, 4, 23), (64, 4, 70)])
def test_flat_manifold_cancels(d, m, D):
    """Known answer (ii): shifted columns inside the column space of J give N = 0 to the N bound while S2 is of order one."""
    cs = SE.flat(d, m, D, 2.0 ** -4)
    N, _, _, st, info = (v[0] for v in run(cs))
    assert info == 0 and st[2] >= 1.0
    ratios = SE.worst_ratios(cs, run(cs))
    print(f"d={d} m={m}: max |N| = {np.abs(N).max():.3e}, trace S2 = {st[2]:.3e}, error / bound = {ratios['N']:.3f}")
    assert ratios["N"] <= 1.0 and np.abs(N).max() <= 1e-10 * st[2]


def test_failures_are_reported_and_confined():
    d, m, D, B = 5, 3, 8, 9
    cs = list(SE.case(B, d, m, D, seed=2))
    clean = run(cs)
    assert (clean[4] == 0).all()
    Jd, jtj, Sd, frame, step, nc = (np.array(v) if isinstance(v, np.ndarray) else v for v in cs)
    Jd[1, :, 2] = 0.0                                                # a zero Jacobian column: the pivot of G fails
    jtj[1, 2, :3] = 0.0
    jtj[1, 2:, 2] = 0.0
    Sd[2 * 2 * m + 3, 4, 1] = NAN                                    # S of sample 2
    Jd[3, 5, 0] = NAN                                                # T of sample 3
    frame[4, 1, 2] = NAN
    jtj[5, 3, 1] = np.inf                                            # a lower triangle
    step[6] = 0.0
    step[7] = NAN
    Jd[7, :, 1] = 0.0                                                # code 2 takes precedence over a failing pivot
    jtj[7, 1, :2] = 0.0
    jtj[7, 1:, 1] = 0.0
    got = run((Jd, jtj, Sd, frame, step, nc))
    assert got[4].tolist() == [0, 1, 2, 2, 2, 2, 2, 2, 0]
    assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all() and np.isnan(got[3][1, 3])
    assert np.isfinite(got[2][1]).all() and np.isfinite(got[3][1, :3]).all()
    for b in range(2, 8):
        assert all(np.isnan(got[i][b]).all() for i in range(4)), b
    for b in (0, 8):
        for a, c in zip(got, clean):
            assert same_bits(a[b], c[b])
    step[6] = -2.0 ** -7
    step[7] = np.inf
    assert run((Jd, jtj, Sd, frame, step, nc))[4].tolist() == [0, 1, 2, 2, 2, 2, 2, 2, 0]


@pytest.mark.parametrize("d,m", [(3, 2), (17, 4), (100, 3)])
def test_position_independence_and_repeatability(d, m):
    Jd, jtj, Sd, frame, step, nc = SE.case(3, d, m, d + 3, seed=3)
    step = np.full(3, 2.0 ** -6)
    where = np.array([0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 2])
    swhere = (where[:, None] * 2 * m + np.arange(2 * m)[None, :]).reshape(-1)
    base = run((Jd, jtj, Sd, frame, step, nc))
    perm = (Jd[where], jtj[where], Sd[swhere], frame[where], step[where], nc)
    first, again = run(perm, "fmajor"), run(perm, "fmajor")
    for a, b, c in zip(base, first, again):
        assert same_bits(a[where], b) and same_bits(b, c)


@pytest.mark.parametrize("B,d,m,D,layout", [(3, 1, 1, 4, "panel"), (2, 17, 4, 20, "fmajor"), (3, 64, 3, 67, "panel"), (2, 128, 4, 131, "fmajor")])
def test_outputs_stay_inside_their_buffers(B, d, m, D, layout):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    q = m * (m + 1) // 2
    cs = SE.case(B, d, m, D, seed=4)
    T, G, S, fr, st = device_inputs(cs, layout)
    bufs = {"second_gram": guarded((B, q, q), torch.float64), "christoffel": guarded((B, q, d), torch.float64),
            "frame_metric": guarded((B, m, m), torch.float64), "stats": guarded((B, 4), torch.float64), "info": guarded((B,), torch.int32)}
    p = lambda name: E._p(bufs[name][1])
    _lib.check(_lib.load().cmf_second_form(E._p(T.data), T.t_b, T.t_r, D, T.nc, d, m, B, E._p(G), E._p(S.data), S.t_b, S.t_r, E._p(fr),
                                           E._p(st), *(p(k) for k in NAMES), E._stream()), "cmf_second_form")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    for got, want in zip((bufs[k][1].cpu().numpy() for k in NAMES), run(cs, layout)):
        assert same_bits(got, want)


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    B, d, m, D = 2, 5, 2, 8
    q = 3
    T, G, S, fr, st = device_inputs(SE.case(B, d, m, D), "panel")
    outs = [torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((B, q, q), (B, q, d), (B, m, m), (B, 4))]
    info = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    ok = [E._p(T.data), T.t_b, T.t_r, D, T.nc, d, m, B, E._p(G), E._p(S.data), S.t_b, S.t_r, E._p(fr), E._p(st), *(E._p(o) for o in outs),
          E._p(info)]
    bad = []
    for i in (0, 8, 9, 12, 13, 14, 15, 16, 17, 18):                  # every pointer NULL, then misaligned
        bad.append((i, None))
        bad.append((i, ok[i].value + (8 if i in (0, 9) else 4 if i in (12, 13, 14, 15, 16, 17) else 2)))
    bad += [(1, T.nc - 4), (1, T.t_b + 2), (2, T.nc - 4), (2, T.t_r + 1), (3, 0), (4, 12), (4, 0), (5, 0), (5, 129), (5, 17), (6, 0), (6, 5),
            (7, 0), (10, 12), (10, S.t_b + 2), (11, 8), (11, S.t_r + 3)]
    for i, value in bad:
        args = list(ok)
        args[i] = value
        assert lib.cmf_second_form(*args, E._stream()) == -1, (i, value)
    args = list(ok)
    args[5], args[6] = 3, 4                                          # m > d
    assert lib.cmf_second_form(*args, E._stream()) == -1
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((info == 7).all())          # nothing was written
    assert lib.cmf_second_form(*ok, E._stream()) == 0
    torch.cuda.synchronize()
    assert info.tolist() == [0, 0]


def test_engine_refusals_empty_call_and_timer():
    from cmf_amd import engine as E
    B, d, m, D = 2, 5, 2, 8
    cs = SE.case(B, d, m, D)
    T, G, S, fr, st = device_inputs(cs, "panel")
    refused = [
        (T, G.cpu(), S, fr, st), (T, G, S, fr.cpu(), st), (T, G, S, fr, st.cpu()),                          # CPU tensors
        (T, G.double(), S, fr, st), (T, G, S, fr.float(), st), (T, G, S, fr, st.float()),                   # dtypes
        (T, G.transpose(1, 2), S, fr, st), (T, G, S, fr.transpose(1, 2).contiguous().transpose(1, 2), st),  # not contiguous
        (T, G, S, fr, torch.zeros(2 * B, dtype=torch.float64, device="cuda")[::2]),
        ("T", G, S, fr, st), (T, G, "S", fr, st),
        (T, G, stack(cs[2][:-1], 16, "panel"), fr, st),                                                     # a shifted sample short
        (T, G, stack(cs[2], 32, "panel"), fr, st),                                                          # not 16 column slots
        (T, G, S, fr[:1].contiguous(), st), (T, G, S, fr, st[:1].contiguous()),
        (T, G, S, torch.zeros(B, 0, d, dtype=torch.float64, device="cuda"), st),                            # m = 0
        (stack(cs[0][:1], 16, "panel"), G, S, fr, st),                                                      # T of another batch
    ]
    for args in refused:
        with pytest.raises(ValueError):
            E.second_form(*args)
    with pytest.raises(ValueError):                                                                         # m = 5 > 4
        c5 = SE.case(1, 6, 4, 9)
        E.second_form(stack(c5[0], 16, "panel"), torch.as_tensor(c5[1]).cuda(), stack(np.zeros((10, 9, 5), np.float32), 16, "panel"),
                      torch.zeros(1, 5, 6, dtype=torch.float64, device="cuda"), torch.as_tensor(c5[4]).cuda())
    with pytest.raises(ValueError):                                                                         # m = 2 > d = 1
        E.second_form(stack(np.ones((1, 4, 1), np.float32), 16, "panel"), torch.ones(1, 1, 1, device="cuda"),
                      stack(np.zeros((4, 4, 2), np.float32), 16, "panel"), torch.ones(1, 2, 1, dtype=torch.float64, device="cuda"),
                      torch.ones(1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):                                                                         # d = 129
        E.second_form(stack(np.zeros((1, 4, 129), np.float32), 144, "panel"), torch.zeros(1, 129, 129, device="cuda"),
                      stack(np.zeros((2, 4, 1), np.float32), 16, "panel"), torch.zeros(1, 1, 129, dtype=torch.float64, device="cuda"),
                      torch.ones(1, dtype=torch.float64, device="cuda"))
    empty = E.second_form(E.Tangent(0, D, 16, "panel", "cuda"), G[:0], E.Tangent(0, D, 16, "panel", "cuda"), fr[:0], st[:0])
    assert empty.second_gram.shape == (0, 3, 3) and empty.christoffel.shape == (0, 3, d) and empty.frame_metric.shape == (0, m, m)
    assert empty.stats.shape == (0, 4) and empty.info.shape == (0,)
    with E.timing(lambda name: True) as t:
        E.second_form(T, G, S, fr, st)
    by = t.by_name()
    assert set(by) == {"second_form"}
