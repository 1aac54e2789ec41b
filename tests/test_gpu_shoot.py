"""Geodesic shooting on the GPU: the metric solve kernel (csrc/shoot_step.hip) against float64 numpy on the same
float32-rounded inputs, its output contract, isolation, determinism and refusals; one evaluation of Hamilton's right-hand side and
whole trajectories against the float64 reference loop (tests/_shoot_reference.py); and ``cmf_amd.ManifoldGeodesic.shoot`` / ``log``
end to end under the conditions tests/test_shoot_host.py establishes.  Needs an MI355X: run with ``-m gpu``.

Kernel bounds, per sample (u = 2^-53):
    solve:  ||G v - p||_inf <= 32 d u (||G||_inf ||v||_inf + ||p||_inf)      the projector's own bound, for the same elimination
    apply:  |out - ref| <= 2 (d + 2) u sum |G| |v|  per element
    stats[0] against recomputation from the outputs: 2 (d + 2) u sum |terms|;  stats[1] = max |out| exactly;  out32 = the correctly
    rounded out64.
The strict upper triangle of every matrix handed to the kernel is NaN.

One evaluation: v, p' and speed2 relative (max-norm) to the float64 reference within the larger of 1e-4 -- the bound
tests/test_gpu_parity.py holds dz_low to -- and 3 x the float32 oracle's own deviation.  Trajectories (S = 8, time 1, the chord
velocity): the end point displacement, the final momentum and the speed2 record within the larger of 3 x the float32 reference
trajectory's deviation and the deviation of the float64 reference with every evaluation scaled by 1 + 1e-4."""
import numpy as np
import pytest
import torch

import _shoot_reference as R
from test_gpu_geodesic import fixture_ends
from test_gpu_metric_stats import build
from test_gpu_projection import guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAN = float("nan")
WIDTHS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128]
BATCHES = [1, 3, 70]


def inputs(B, d, seed=0, cond=1e3):
    """(G (B, d, d) float32 whose strict upper triangle is NaN, its symmetric float64 value, rhs (B, d) float64): SPD matrices
    Q diag(s) Q^T with s from 1 down to 1 / cond, built in float64 and rounded."""
    gen = torch.Generator().manual_seed(1000 * d + B + seed)
    Q = torch.linalg.qr(torch.randn(B, d, d, generator=gen, dtype=torch.float64))[0]
    s = torch.logspace(0, -np.log10(cond), d, dtype=torch.float64) if d > 1 else torch.ones(1, dtype=torch.float64)
    scale = 2.0 ** torch.randint(-3, 4, (B, 1, 1), generator=gen).double()
    G = ((Q * s) @ Q.transpose(1, 2) * scale).float().numpy()
    low = np.tril(np.ones((d, d), dtype=bool))
    G = np.where(low, G, np.transpose(G, (0, 2, 1)))                 # symmetric in float32: the lower triangle decides
    rhs = torch.randn(B, d, generator=gen, dtype=torch.float64).numpy()
    return np.where(low, G, np.float32(NAN)), G.astype(np.float64), rhs


def run(G, rhs, apply=False):
    """``engine.metric_solve`` on CPU inputs -> numpy (out64, out32, stats, info)."""
    from cmf_amd import engine as E
    r = E.metric_solve(torch.as_tensor(G).cuda(), torch.as_tensor(rhs).cuda(), apply=apply)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (r.out64, r.out32, r.stats, r.info))


def check_common(rhs, out64, out32, stats, info, d, label):
    assert (info == 0).all(), label
    assert out64.dtype == np.float64 and out32.dtype == np.float32 and stats.dtype == np.float64 and info.dtype == np.int32
    assert same_bits(out32, out64.astype(np.float32)), label
    terms = rhs * out64
    assert (np.abs(stats[:, 0] - terms.sum(1)) <= 2 * (d + 2) * U * np.abs(terms).sum(1)).all(), label
    assert same_bits(stats[:, 1], np.abs(out64).max(1)), label


@pytest.mark.parametrize("d", WIDTHS)
def test_solve_matches_float64(d):
    for B in BATCHES:
        G, G64, p = inputs(B, d)
        v, v32, stats, info = run(G, p)
        check_common(p, v, v32, stats, info, d, f"B={B}")
        res = np.abs(np.einsum("bij,bj->bi", G64, v) - p).max(1)
        scale = np.abs(G64).sum(2).max(1) * np.abs(v).max(1) + np.abs(p).max(1)
        print(f"d={d} B={B}: worst residual / (d 2^-53 scale) = {float((res / (d * U * scale)).max()):.3f} (bound 32)")
        assert (res <= 32 * d * U * scale).all()
        assert (stats[:, 0] > 0).all()                               # the squared speed of an SPD metric


@pytest.mark.parametrize("d", WIDTHS)
def test_apply_matches_float64(d):
    for B in BATCHES:
        G, G64, v = inputs(B, d, seed=1)
        p, p32, stats, info = run(G, v, apply=True)
        check_common(v, p, p32, stats, info, d, f"B={B}")
        ref = np.einsum("bij,bj->bi", G64, v)
        mag = np.einsum("bij,bj->bi", np.abs(G64), np.abs(v))
        print(f"d={d} B={B}: max err / bound = {float((np.abs(p - ref) / (2 * (d + 2) * U * mag)).max()):.3f}")
        assert (np.abs(p - ref) <= 2 * (d + 2) * U * mag).all()


@pytest.mark.parametrize("apply", [False, True])
def test_failures_are_reported_and_confined(apply):
    d = 5
    G, _, rhs = inputs(7, d, seed=2)
    clean = run(G, rhs, apply)
    assert (clean[3] == 0).all()
    G[1, 2, 2] = -1.0                                                # a negative pivot
    G[3, 4, 1] = NAN                                                 # the lower triangle
    rhs[4, 0] = np.inf
    out64, out32, stats, info = run(G, rhs, apply)
    assert info.tolist() == ([0, 0, 0, 2, 2, 0, 0] if apply else [0, 1, 0, 2, 2, 0, 0])
    for b in (3, 4) if apply else (1, 3, 4):
        assert np.isnan(out64[b]).all() and np.isnan(out32[b]).all() and np.isnan(stats[b]).all()
    others = [0, 2, 5, 6]
    for got, want in zip((out64, out32, stats), clean):
        assert same_bits(got[others], want[others])
    if apply:                                                        # a product has no pivots: an indefinite matrix is applied
        assert np.isfinite(out64[1]).all() and np.isfinite(stats[1]).all()


@pytest.mark.parametrize("d", [3, 17, 100])
def test_position_independence_and_repeatability(d):
    G, G64, rhs = inputs(3, d, seed=3)
    where = [0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 2]
    for apply in (False, True):
        base = run(G, rhs, apply)
        batch = run(G[where], rhs[where], apply)
        again = run(G[where], rhs[where], apply)
        for a, b, c in zip(base, batch, again):
            assert same_bits(a[where], b) and same_bits(b, c)
        # the strict upper triangle is never read: NaN there (above) and the symmetric values give the same bits
        for a, b in zip(base, run(G64.astype(np.float32), rhs, apply)):
            assert same_bits(a, b)


@pytest.mark.parametrize("B,d", [(3, 1), (2, 17), (3, 64), (2, 128)])
def test_outputs_stay_inside_their_buffers(B, d):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    G, _, rhs = inputs(B, d, seed=4)
    Gc, rc = torch.as_tensor(G).cuda(), torch.as_tensor(rhs).cuda()
    lib = _lib.load()
    for apply in (0, 1):
        bufs = {"out64": guarded((B, d), torch.float64), "out32": guarded((B, d), torch.float32),
                "stats": guarded((B, 2), torch.float64), "info": guarded((B,), torch.int32)}
        p = lambda name: E._p(bufs[name][1])
        _lib.check(lib.cmf_metric_solve(E._p(Gc), E._p(rc), d, B, apply, p("out64"), p("out32"), p("stats"), p("info"), E._stream()),
                   "cmf_metric_solve")
        torch.cuda.synchronize()
        for buf, _, fill in bufs.values():
            assert guards_intact(buf, fill)
        want = run(G, rhs, bool(apply))
        for name, w in zip(("out64", "out32", "stats", "info"), want):
            assert same_bits(bufs[name][1].cpu().numpy(), w)


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    B, d = 2, 3
    G, _, rhs = inputs(B, d)
    Gc, rc = torch.as_tensor(G).cuda(), torch.as_tensor(rhs).cuda()
    out64, out32 = torch.empty(B, d, dtype=torch.float64, device="cuda"), torch.empty(B, d, device="cuda")
    stats, info = torch.empty(B, 2, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    ok = [E._p(Gc), E._p(rc), d, B, 0, E._p(out64), E._p(out32), E._p(stats), E._p(info)]
    assert lib.cmf_metric_solve(*ok, E._stream()) == 0
    for i, value in ((0, None), (1, None), (2, 0), (2, 129), (3, 0), (4, 2), (4, -1), (5, None), (6, None), (7, None), (8, None)):
        args = list(ok)
        args[i] = value
        assert lib.cmf_metric_solve(*args, E._stream()) == -1, (i, value)
    import ctypes as C
    for i in (1, 5, 7):                                              # float64 pointers: 8-byte aligned
        args = list(ok)
        args[i] = C.c_void_p(args[i].value + 4)
        assert lib.cmf_metric_solve(*args, E._stream()) == -1, i
    torch.cuda.synchronize()


def test_engine_refusals_and_timer_entry():
    from cmf_amd import engine as E
    assert E.SHOOT_MAX_WIDTH == 128
    G, _, rhs = inputs(2, 3)
    Gc, rc = torch.as_tensor(np.nan_to_num(G)).cuda(), torch.as_tensor(rhs).cuda()
    with pytest.raises(ValueError, match="GPU"):
        E.metric_solve(Gc.cpu(), rc)
    with pytest.raises(ValueError, match="GPU"):
        E.metric_solve(Gc, rc.cpu())
    with pytest.raises(ValueError, match="float32"):
        E.metric_solve(Gc.double(), rc)
    with pytest.raises(ValueError, match="float64"):
        E.metric_solve(Gc, rc.float())
    with pytest.raises(ValueError, match="contiguous"):
        E.metric_solve(Gc.transpose(1, 2), rc)
    with pytest.raises(ValueError, match="contiguous"):
        E.metric_solve(Gc, rc.t().contiguous().t())
    with pytest.raises(ValueError, match="rhs must be"):
        E.metric_solve(Gc, rc[:, :2].contiguous())
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.metric_solve(torch.zeros(1, 129, 129, device="cuda"), torch.zeros(1, 129, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.metric_solve(torch.zeros(1, 0, 0, device="cuda"), torch.zeros(1, 0, dtype=torch.float64, device="cuda"))
    r = E.metric_solve(Gc[:0], rc[:0])                               # no sample: empties, no launch
    assert r.out64.shape == (0, 3) and r.out32.shape == (0, 3) and r.stats.shape == (0, 2) and r.info.shape == (0,)
    assert r.out64.dtype == torch.float64 and r.out32.dtype == torch.float32 and r.info.dtype == torch.int32
    with E.timing(lambda name: True) as timer:
        E.metric_solve(Gc, rc)
        E.metric_solve(Gc, rc, apply=True)
    by = timer.by_name()
    assert set(by) == {"metric_solve"}
    n, ms, flops, nbytes = by["metric_solve"]
    assert n == 2 and ms >= 0 and flops > 0 and nbytes > 0


# --------------------------------------------------------------------------------------------------
# one evaluation and whole trajectories against the float64 reference
# --------------------------------------------------------------------------------------------------


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())


def geodesic(dens, **kw):
    import cmf_amd
    return cmf_amd.ManifoldGeodesic(dens, **kw)


def pool(head):
    from cmf_amd import engine as E
    return E.GradPool([q for q in head.parameters() if q.requires_grad], "cuda")


@pytest.mark.parametrize("name", R.FIXTURES + ["c3_mnist_full"])
def test_one_evaluation_matches_the_float64_reference(name):
    g, meta, dens, head, x = build(name)
    model, model32 = R.model_of(name), R.model_of(name, torch.float32)
    n = 1 if name == "c3_mnist_full" else 4                        # the full-size oracle in float64 costs seconds per sample
    with torch.no_grad():
        z = model.encode(model.y[:n]).float()
    p = torch.randn(z.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    want = R.evaluate(model, z.double(), p)
    yard = R.evaluate(model32, z, p.float())
    marker = object()
    head.last_gram = head.last_hutchinson = marker
    dp, v, s2, info, x_hat = geodesic(dens).shoot_evaluate(z.cuda(), p.cuda(), pool(head))
    assert head.last_gram is marker and head.last_hutchinson is marker
    assert dp.dtype == v.dtype == s2.dtype == torch.float64 and dp.shape == v.shape == z.shape and s2.shape == (len(z),)
    assert bool((info == 0).all())
    for label, got, ref, ref32 in zip(("p'", "v", "speed2"), (dp, v, s2), want, yard):
        bound = max(1e-4, 3.0 * rel(ref32, ref))
        print(f"{name}: {label}: rel {rel(got, ref):.2e} (float32 oracle {rel(ref32, ref):.2e}, bound {bound:.2e})")
        assert rel(got, ref) <= bound, label
    with torch.no_grad():
        assert rel(x_hat.flatten(1), model.decode(z.double()).flatten(1)) <= 1e-4


@pytest.mark.parametrize("name", R.FIXTURES)
def test_trajectories_match_the_float64_reference(name):
    g, meta, dens, head, x = build(name)
    model, z0, z1, ref = R.chord_run(name)
    ref32 = R.chord_run(name, torch.float32)[3]
    scaled = R.chord_run(name, scale=1.0 + 1e-4)[3]
    out = geodesic(dens).shoot_latents(z0.float().cuda(), (z1 - z0).cuda(), steps=R.STEPS)
    B, S, d = z0.shape[0], R.STEPS, z0.shape[1]
    assert out["latents"].shape == (B, S + 1, d) and out["latents"].dtype == torch.float32
    for key in ("velocity", "momentum"):
        assert out[key].shape == (B, S + 1, d) and out[key].dtype == torch.float64
    assert out["speed2"].shape == (B, S + 1) and out["speed2"].dtype == torch.float64
    assert out["length"].shape == (B,) and out["length"].dtype == torch.float64
    assert out["path_head"].shape == (B, S + 1, *head.x_shape)
    assert out["steps_taken"].dtype == torch.int32 and out["info"].dtype == torch.int32
    assert bool((out["info"] == 0).all()) and bool((out["steps_taken"] == S).all())
    assert all(t.is_cuda for t in out.values())
    assert torch.equal(out["latents"][:, 0], z0.float().cuda())
    pick = {"displacement": lambda o: o["latents"][:, -1].double().cpu() - z0, "momentum": lambda o: o["momentum"][:, -1],
            "speed2": lambda o: o["speed2"]}
    for label, f in pick.items():
        bound = max(3.0 * rel(f(ref32), f(ref)), rel(f(scaled), f(ref)))
        print(f"{name}: {label}: rel {rel(f(out), f(ref)):.2e} (float32 reference {rel(f(ref32), f(ref)):.2e}, scaled "
              f"{rel(f(scaled), f(ref)):.2e}, bound {bound:.2e})")
        assert rel(f(out), f(ref)) <= bound, label
    s = out["speed2"].sqrt()
    assert torch.allclose(out["length"], (0.5 * (s[:, :-1] + s[:, 1:])).sum(1) / S, rtol=1e-14, atol=0)
    with torch.no_grad():                                            # DESIGN 5's x_hat tolerance between two float32 decodes
        assert rel(out["path_head"].flatten(0, 1), head.flow_forward(out["latents"].flatten(0, 1))) <= 1e-5


# --------------------------------------------------------------------------------------------------
# the product
# --------------------------------------------------------------------------------------------------


def product_ends(name, x):
    return (x[:1].contiguous(), x[1:2].contiguous()) if name == "mini_cifar" else fixture_ends(name, x)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_shooting_the_logarithm_arrives(name):
    g, meta, dens, head, x = build(name)
    x0, x1 = product_ends(name, x)
    geo = geodesic(dens, points=9, steps=10, shoot_steps=R.STEPS)
    keep0, marker = x0.clone(), object()
    head.last_gram = marker
    lg = geo.log(x0, x1)
    out = geo.shoot(x0, lg["velocity"])
    assert head.last_gram is marker and torch.equal(x0, keep0)
    B = x0.shape[0]
    assert lg["velocity"].shape == (B, head.program.d) and lg["velocity"].dtype == torch.float64
    assert out["path"].shape == (B, R.STEPS + 1, *x0.shape[1:]) and bool((out["info"] == 0).all())
    miss = (out["path_head"][:, -1] - lg["path_head"][:, -1]).flatten(1).double().norm(dim=1)
    ratio = miss / lg["length"]
    speed = out["speed2"][:, 0].sqrt() / lg["length"]
    print(f"{name}: miss / length in [{float(ratio.min()):.2e}, {float(ratio.max()):.2e}]; sqrt(speed2_0) / length in "
          f"[{float(speed.min()):.4f}, {float(speed.max()):.4f}]")
    assert bool((ratio <= 2e-2).all())
    if name in R.MLP:
        z0, z1 = lg["latents"][:, 0].contiguous(), lg["latents"][:, -1]
        chord = geo.shoot_latents(z0, (z1.double() - z0.double()))
        chord_miss = (chord["path_head"][:, -1] - lg["path_head"][:, -1]).flatten(1).double().norm(dim=1)
        print(f"{name}: miss over the straight chord's max {float((miss / chord_miss).max()):.3f}")
        assert bool((miss <= 0.1 * chord_miss).all())
    if name == "mini_mnist":                                         # the same in data space, through ``path``
        seg = (lg["path"][:, 1:] - lg["path"][:, :-1]).flatten(2).double().norm(dim=2).sum(1)
        data = (out["path"][:, -1] - lg["path"][:, -1]).flatten(1).double().norm(dim=1) / seg
        print(f"{name}: data space miss / length max {float(data.max()):.2e}")
        assert bool((data <= 2e-2).all())


def test_log_is_connect_plus_the_velocity():
    g, meta, dens, head, x = build("c2a_power")
    x0, x1 = fixture_ends("c2a_power", x)
    geo = geodesic(dens, points=6, steps=3)
    con, lg = geo.connect(x0, x1), geo.log(x0, x1)
    assert set(lg) == set(con) | {"velocity"} and "velocity" not in con
    assert all(torch.equal(lg[k], con[k]) for k in con)
    z = lg["latents"].double()
    assert torch.equal(lg["velocity"], 5 * (-3.0 * z[:, 0] + 4.0 * z[:, 1] - z[:, 2]) / 2.0)
    same = geo.log_latents(lg["latents"][:, 0].contiguous(), lg["latents"][:, -1].contiguous())
    assert all(torch.equal(same[k], lg[k]) for k in lg)


def three_starts(name):
    g, meta, dens, head, x = build(name)
    model, z0, z1 = R.ends(name)
    return dens, head, z0[:3].float().cuda().contiguous(), (z1 - z0)[:3].cuda().contiguous()


def test_sub_batches_give_the_trajectories_of_one_call(monkeypatch):
    from cmf_amd import engine as E
    dens, head, z0, v0 = three_starts("c2a_power")
    geo = geodesic(dens)
    whole = geo.shoot_latents(z0, v0, steps=4)
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(3) == 1                               # three sub-batches of one trajectory
    pieces = geo.shoot_latents(z0, v0, steps=4)
    assert set(pieces) == set(whole)
    for key in whole:
        assert pieces[key].shape == whole[key].shape and torch.equal(pieces[key], whole[key]), key


def test_a_failed_trajectory_freezes_alone():
    dens, head, z0, v0 = three_starts("c2a_power")
    geo, S = geodesic(dens), 4
    bad = z0.clone()
    bad[1, 0] = NAN
    out = geo.shoot_latents(bad, v0, steps=S)
    assert out["info"].tolist() == [0, 2, 0] and out["steps_taken"].tolist() == [S, 0, S]
    assert bool(torch.isnan(out["speed2"][1]).all()) and float(out["length"][1]) == 0.0
    assert torch.equal(out["latents"][1, 1:].isnan(), out["latents"][1, :1].isnan().expand(S, -1))      # every node repeats node 0
    alone = geo.shoot_latents(z0[[0, 2]].contiguous(), v0[[0, 2]].contiguous(), steps=S)
    for key in out:
        assert torch.equal(out[key][[0, 2]], alone[key]), key


def test_validation():
    dens, head, z0, v0 = three_starts("c2a_power")
    import cmf_amd
    geo = geodesic(dens)
    with pytest.raises(ValueError, match="shoot_steps"):
        cmf_amd.ManifoldGeodesic(dens, shoot_steps=0)
    with pytest.raises(ValueError, match="must both be"):
        geo.shoot_latents(z0, v0[:2])
    with pytest.raises(ValueError, match="must both be"):
        geo.shoot_latents(z0[:, :1].contiguous(), v0[:, :1].contiguous())
    with pytest.raises(ValueError, match="must both be"):
        geo.shoot_latents(z0, v0.cpu())
    with pytest.raises(ValueError, match="steps >= 1"):
        geo.shoot_latents(z0, v0, steps=0)
    with pytest.raises(ValueError, match="at least one"):
        geo.shoot_latents(z0[:0], v0[:0])
    for time in (0.0, -1.0, float("inf"), NAN):
        with pytest.raises(ValueError, match="time"):
            geo.shoot_latents(z0, v0, time=time)
    g, meta, dens, head, x = build("c2a_power")
    with pytest.raises(ValueError, match="at least one"):
        geo.shoot(x[:0], v0[:0])
    with pytest.raises(RuntimeError, match="CPU fallback"):
        geo.shoot(x[:3].cpu(), v0)
    half = geo.shoot_latents(z0, v0, steps=2, time=0.5)
    full = geo.shoot_latents(z0, v0, steps=4, time=1.0)
    assert torch.equal(half["latents"], full["latents"][:, :3])     # equal steps: a prefix of the same loop
