"""The metric spectrum on the GPU: the Jacobi kernel (csrc/gram_spectrum.hip) against ``torch.linalg.eigvalsh`` in float64 on the
same float32 input (which reads the lower triangle like the kernel), its output contract, determinism and input validation, and
``cmf_amd.MetricSpectrum`` end to end against the reference-generated fixtures.  Needs an MI355X: run with ``-m gpu``.

Kernel bounds, per sample, with C = 32 (tests/_jacobi_emulation.BOUND_C):
    |lambda - lambda_ref| <= C d 2^-53 max |lambda_ref|,  max |G V - V Lambda| <= C d 2^-53 max |lambda_ref|,  max |V^T V - I| <= C d 2^-53
-- the form backward stability gives; tests/test_metric_spectrum_host.py holds a float64 emulation of the kernel's operation
sequence on the same inputs to a quarter of them (worst ratio to d 2^-53 there: 7.1).  One float32 operation anywhere in a
rotation would land near 2^-24, five orders of magnitude outside."""
import json
import os

import numpy as np
import pytest
import torch

import _jacobi_emulation as J
from conftest import COND, SMALL, kink_tolerance
from test_gpu_metric_stats import build, prior_jacobians

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 64
NAN = float("nan")
RECORDED_SWEEPS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jacobi_emulation_sweeps.json")))


def spectrum(G, vectors):
    """``engine.gram_spectrum`` on a CPU float32 batch -> the record with CPU tensors."""
    from cmf_amd import engine as E
    r = E.gram_spectrum(G.cuda(), vectors=vectors)
    torch.cuda.synchronize()
    for name in ("eigenvalues", "vectors", "sweeps", "info"):
        t = getattr(r, name)
        setattr(r, name, None if t is None else t.cpu())
    return r


def same(a, b, rows_a=None, rows_b=None):
    """Bit identity of two records (optionally of a selection of samples); NaN outputs compare by position."""
    for name in ("eigenvalues", "vectors", "sweeps", "info"):
        x, y = getattr(a, name), getattr(b, name)
        if x is None or y is None:
            if x is not y:
                return False
            continue
        x, y = (x if rows_a is None else x[rows_a]), (y if rows_b is None else y[rows_b])
        if not torch.equal(torch.nan_to_num(x.double(), nan=12345.0), torch.nan_to_num(y.double(), nan=12345.0)) or \
                not torch.equal(torch.isnan(x.double()), torch.isnan(y.double())):
            return False
    return True


@pytest.mark.parametrize("B,d", J.SHAPES)
def test_kernel_matches_float64_eigvalsh(B, d):
    labels, G = J.cases(B, d)
    ref = torch.linalg.eigvalsh(G.double())
    plain, full = spectrum(G, False), spectrum(G, True)
    print(f"B={B} d={d}: sweeps {dict(zip(labels, full.sweeps.tolist()))}; the emulation's {RECORDED_SWEEPS[f'{B}x{d}']}")
    assert torch.equal(plain.eigenvalues, full.eigenvalues) and torch.equal(plain.sweeps, full.sweeps)        # the same bits
    assert plain.vectors is None and full.vectors.shape == (len(labels), d, d) and full.vectors.dtype == torch.float64
    for r in (plain, full):
        e_val, e_res, e_orth = J.error_ratios(G.numpy(), r.eigenvalues.numpy(), None if r.vectors is None else r.vectors.numpy(),
                                              ref=ref.numpy())
        print(f"  ratios to d 2^-53 (bound {J.BOUND_C:g}): eigenvalues {e_val.max():.2f}"
              + ("" if e_res is None else f", residual {e_res.max():.2f}, orthogonality {e_orth.max():.2f}"))
        assert (e_val <= J.BOUND_C).all()
        if r.vectors is not None:
            assert (e_res <= J.BOUND_C).all() and (e_orth <= J.BOUND_C).all()
            assert J.sign_rule_holds(r.vectors.numpy())
        assert bool((r.info == 0).all()) and bool((r.sweeps >= 1).all()) and bool((r.sweeps <= J.MAX_SWEEPS).all())
        assert bool((r.eigenvalues[:, 1:] >= r.eigenvalues[:, :-1]).all())
        for name in ("identity", "repeated_diagonal", "zero"):
            assert int(r.sweeps[labels.index(name)]) == 1
    k = labels.index("repeated_diagonal")
    assert torch.equal(full.eigenvalues[k], torch.diagonal(G[k]).double().sort().values)
    if d >= 4:                       # equal values keep the order of their diagonal positions: the 1s sit at 1, 3, 5, ...
        assert torch.equal(full.vectors[k][:, 0], torch.eye(d, dtype=torch.float64)[:, 1])
        assert torch.equal(full.vectors[k][:, 1], torch.eye(d, dtype=torch.float64)[:, 3])
    assert torch.equal(full.vectors[labels.index("zero")], torch.eye(d, dtype=torch.float64))


def guarded(shape, dtype):
    """A view of ``shape`` between two guard bands of a recognisable fill: (whole buffer, the view, the fill)."""
    n = int(np.prod(shape))
    fill = NAN if dtype.is_floating_point else -77
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape), fill


def guards_intact(buf, fill):
    edge = torch.cat((buf[:GUARD], buf[-GUARD:]))
    return bool(torch.isnan(edge).all()) if buf.dtype.is_floating_point else bool((edge == fill).all())


@pytest.mark.parametrize("B,d", [(3, 17), (2, 64), (3, 100)])
@pytest.mark.parametrize("vectors", [False, True])
def test_outputs_stay_inside_their_buffers(B, d, vectors):
    from cmf_amd import _lib
    from cmf_amd import engine as E
    G = J.gram(B, d).cuda()
    bufs = {"eig": guarded((B, d), torch.float64), "sweeps": guarded((B,), torch.int32), "info": guarded((B,), torch.int32)}
    if vectors:
        bufs["vec"] = guarded((B, d, d), torch.float64)
    p = lambda name: E._p(bufs[name][1]) if name in bufs else None
    _lib.check(_lib.load().cmf_gram_spectrum(E._p(G), d, B, p("eig"), p("vec"), p("sweeps"), p("info"), E._stream()), "cmf_gram_spectrum")
    torch.cuda.synchronize()
    for buf, _, fill in bufs.values():
        assert guards_intact(buf, fill)
    want = spectrum(G.cpu(), vectors)
    assert torch.equal(bufs["eig"][1].cpu(), want.eigenvalues) and torch.equal(bufs["sweeps"][1].cpu(), want.sweeps)
    assert bool((bufs["info"][1] == 0).all())
    if vectors:
        assert torch.equal(bufs["vec"][1].cpu(), want.vectors)


def test_entry_point_refuses_bad_arguments():
    from cmf_amd import _lib
    from cmf_amd import engine as E
    lib = _lib.load()
    G = J.gram(2, 3).cuda()
    eig = torch.zeros(2 * 3 + 1, dtype=torch.float64, device="cuda")
    vec = torch.zeros(2 * 9, dtype=torch.float64, device="cuda")
    sw, info = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    odd = eig.view(torch.float32)[1:]                                                  # 4 bytes past an 8-byte boundary
    ok = (E._p(G), 3, 2, E._p(eig), E._p(vec), E._p(sw), E._p(info))
    for i, bad in ((0, None), (3, None), (5, None), (6, None), (1, 0), (1, 129), (2, 0), (3, E._p(odd)), (4, E._p(odd))):
        args = list(ok)
        args[i] = bad
        assert lib.cmf_gram_spectrum(*args, E._stream()) == -1
    torch.cuda.synchronize()
    assert float(eig.abs().sum()) == 0.0 and float(vec.abs().sum()) == 0.0 and int(sw.sum()) == 0


@pytest.mark.parametrize("d", [17, 100])
def test_position_independence_and_repeatability(d):
    labels, G = J.cases(2, d)
    base = G[[0, labels.index("two_clusters"), labels.index("geometric_1e12")]].contiguous()
    where = [0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 2]
    batch = base[where].contiguous()
    for vectors in (False, True):
        want, got = spectrum(base, vectors), spectrum(batch, vectors)
        assert same(got, want, rows_b=where)
        assert same(spectrum(batch, vectors), got)
        upper = torch.triu(torch.ones(d, d, dtype=torch.bool), 1)
        assert same(spectrum(torch.where(upper, torch.full_like(batch, NAN), batch), vectors), got)


@pytest.mark.parametrize("d", [10, 100])
def test_non_finite_samples_are_reported_and_isolated(d):
    G = J.gram(6, d, seed=4)
    clean = spectrum(G, True)
    dirty = G.clone()
    dirty[1, 3, 1] = NAN
    dirty[4, d - 1, d - 1] = float("inf")
    dirty[2, 1, 3] = NAN                                     # the upper triangle is never read: sample 2 stays valid
    for vectors in (False, True):
        got = spectrum(dirty, vectors)
        assert got.info.tolist() == [0, 2, 0, 0, 2, 0] and got.sweeps[[1, 4]].tolist() == [0, 0]
        assert bool(torch.isnan(got.eigenvalues[[1, 4]]).all())
        if vectors:
            assert bool(torch.isnan(got.vectors[[1, 4]]).all())
            assert same(got, clean, rows_a=[0, 2, 3, 5], rows_b=[0, 2, 3, 5])
        else:
            assert torch.equal(got.eigenvalues[[0, 2, 3, 5]], clean.eigenvalues[[0, 2, 3, 5]])


def test_engine_refusals():
    from cmf_amd import engine as E
    with pytest.raises(ValueError, match="1 <= d <= 128"):
        E.gram_spectrum(torch.zeros(1, 129, 129, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        E.gram_spectrum(J.gram(2, 3).cuda().transpose(1, 2))
    with pytest.raises(ValueError, match="contiguous"):
        E.gram_spectrum(torch.zeros(2, 3, 4, device="cuda"))
    with pytest.raises(ValueError, match="float32"):
        E.gram_spectrum(J.gram(2, 3).double().cuda())
    with pytest.raises(ValueError, match="GPU"):
        E.gram_spectrum(J.gram(2, 3))


# --------------------------------------------------------------------------------------------------
# end to end against the fixtures
# --------------------------------------------------------------------------------------------------


def run_update(dens, head, x, coordinates="latent", vectors=False):
    """One ``update`` with the side-effect checks every end-to-end case makes: x untouched, ``last_gram`` left alone."""
    import cmf_amd
    spec = cmf_amd.MetricSpectrum(dens, coordinates=coordinates, vectors=vectors)
    keep, marker = x.clone(), object()
    head.last_gram = marker
    out = spec.update(x)
    assert head.last_gram is marker and torch.equal(x, keep)
    B, d = x.shape[0], head.program.d
    assert out["eigenvalues"].shape == (B, d) and out["eigenvalues"].is_cuda and out["eigenvalues"].dtype == torch.float64
    for key in ("info", "sweeps", "log_volume", "condition", "participation_ratio"):
        assert out[key].shape == (B,) and out[key].is_cuda
    assert ("vectors" in out) == vectors
    return spec, out


def check_against(out, G_ref, tol, label):
    """Eigenvalues against ``eigvalsh`` of the reference's float64 Gram matrices, whose own tolerance is ``tol`` relative to
    max |G_b|: Weyl's inequality, |delta lambda_k| <= ||E||_2 <= d max |E_ij| = d tol max |G_b|; the log-volume against half the
    reference's log-determinant at the project's log-det tolerance (max-norm relative, like tests/test_gpu_parity.rel)."""
    G = G_ref.double()
    d = G.shape[1]
    ref = torch.linalg.eigvalsh(G)
    err = (out["eigenvalues"].cpu() - ref).abs().max(1).values
    bound = d * tol * G.abs().reshape(len(G), -1).max(1).values
    half_logdet = 0.5 * torch.linalg.slogdet(G).logabsdet
    lv = out["log_volume"].cpu()
    rel_lv = float((lv - half_logdet).abs().max() / half_logdet.abs().max().clamp_min(1e-9))
    print(f"{label}: d={d} eigenvalue err/bound {float((err / bound).max()):.3e}; log_volume rel {rel_lv:.2e} (tol {tol:.2e}); sweeps "
          f"{out['sweeps'].tolist()}; condition max {float(out['condition'].max()):.3e}")
    assert bool((out["info"] == 0).all())
    assert bool((err <= bound).all())
    assert rel_lv <= tol
    lam = out["eigenvalues"].cpu()
    assert torch.equal(out["condition"].cpu(), lam[:, -1] / lam[:, 0])
    pr = lam.sum(1) ** 2 / (lam * lam).sum(1)
    assert bool(((out["participation_ratio"].cpu() - pr).abs() <= 8 * d * U * pr).all())


@pytest.mark.parametrize("name", SMALL + COND + ["c3_mnist_full"])
def test_latent_coordinates_match_the_fixture(name):
    from cmf_amd import engine as E
    g, meta, dens, head, x = build(name)
    if head.program.d > E.SPECTRUM_MAX_WIDTH:
        pytest.skip(f"{name}: latent dimension {head.program.d} > {E.SPECTRUM_MAX_WIDTH}, the widest the spectrum kernel takes")
    spec, out = run_update(dens, head, x)
    check_against(out, g["jtj"], kink_tolerance(g), name)
    r = spec.result()
    assert r["count"] == x.shape[0] and r["skipped"] == 0


@pytest.mark.parametrize("name", ["c2a_power", "mini_mnist"])
def test_noise_coordinates_match_the_fixture(name):
    g, meta, dens, head, x = build(name)
    P = prior_jacobians(meta, g["earliest_latent"])
    G_ref = P.transpose(1, 2) @ g["jtj"].double() @ P
    spec, out = run_update(dens, head, x, "noise", vectors=True)
    check_against(out, G_ref, kink_tolerance(g), name + " (noise)")
    V, lam = out["vectors"].cpu(), out["eigenvalues"].cpu()
    d = V.shape[1]
    assert bool(((V.transpose(1, 2) @ V - torch.eye(d, dtype=torch.float64)).abs() <= J.BOUND_C * d * U).all())


def test_streaming_equals_one_update():
    """Two updates of half batches against the whole batch.  With halves of ONE sample each both states are the same two-term sums, so they
    agree within the 4 * 2^-53 relative per entry of a two-term re-association.  With halves of n > 1 samples the two sums of
    2 n terms are taken in different orders; any order is within (2 n - 1) 2^-53 sum |term| of the exact sum, so they differ by at
    most 2 (2 n - 1) 2^-53 sum |term| -- asserted with sum |term| from the per-sample outputs."""
    import cmf_amd
    # the two fixtures tests/test_gpu_metric_stats.py streams in sub-batches: their decode sweep gives a sample the same Gram
    # matrix in every batch it is part of
    for name, n in (("mini_mnist", 1), ("c2a_power", 16)):
        g, meta, dens, head, x = build(name)
        d = head.program.d
        label, a, b = f"{name} {n} + {n}", x[:n], x[n:2 * n]
        whole, out = run_update(dens, head, torch.cat((a, b)).contiguous())
        halves = cmf_amd.MetricSpectrum(dens)
        o1, o2 = halves.update(a.contiguous()), halves.update(b.contiguous())
        assert torch.equal(torch.cat((o1["eigenvalues"], o2["eigenvalues"])), out["eigenvalues"])
        w, h = whole.state.flat.cpu(), halves.state.flat.cpu()
        lam = out["eigenvalues"].cpu()
        terms = torch.cat((lam.log().abs().sum(0), lam.abs().sum(0), out["participation_ratio"].cpu().abs().sum().reshape(1)))
        diff = (w - h).abs()
        print(f"{label}: max |whole - halves| / (2^-53 |entry|) = {float((diff / (U * w.abs()).clamp_min(1e-300)).max()):.2f}")
        assert torch.equal(w[-2:], h[-2:]) and float(w[-2]) == a.shape[0] + b.shape[0] and float(w[-1]) == 0
        if a.shape[0] == 1:
            assert bool((diff <= 4 * U * w.abs()).all())
        assert bool((diff[:-2] <= 2 * (2 * a.shape[0] - 1) * U * terms).all())
        # the mean log-volume is the mean of the per-sample log-volumes: the same B d terms 1/2 log lambda in another order
        lv = out["log_volume"].cpu()
        B = lv.numel()
        r = whole.result()
        assert abs(r["mean_log_volume"] - float(lv.mean())) <= 2 * (B * d + 2) * U * float(0.5 * lam.log().abs().sum()) / B
        assert r["count"] == B


def test_an_invalid_sample_is_skipped_not_counted():
    from cmf_amd import engine as E
    from cmf_amd.metric_spectrum import SpectrumState, accumulate, summarize
    G = J.gram(4, 5, seed=9)
    G[2, 4, 0] = NAN
    r = E.gram_spectrum(G.cuda())
    state = SpectrumState(5, device="cuda")
    out = summarize(r.eigenvalues, r.info)
    accumulate(state.flat, out)
    res = state.result()
    assert res["count"] == 3 and res["skipped"] == 1
    assert out["valid"].tolist() == [True, True, False, True]
    assert bool(torch.isnan(out["log_volume"][2])) and bool(torch.isnan(out["condition"][2]))
    keep = [0, 1, 3]
    assert torch.allclose(res["mean_eigenvalues"], r.eigenvalues[keep].cpu().mean(0), rtol=1e-14, atol=0)
    # a singular metric is a legitimate result, but not a valid sample: its log-volume does not exist
    rz = E.gram_spectrum(torch.zeros(1, 5, 5, device="cuda"))
    oz = summarize(rz.eigenvalues, rz.info)
    accumulate(state.flat, oz)
    assert state.result()["count"] == 3 and state.result()["skipped"] == 2 and int(rz.info[0]) == 0
    assert float(oz["condition"][0]) == float("inf") and bool(torch.isnan(oz["log_volume"][0]))


def test_metric_statistics_are_untouched():
    import cmf_amd
    g, meta, dens, head, x = build("mini_mnist")
    before = cmf_amd.MetricStatistics(dens)
    macs_before = before.update(x)
    spec = cmf_amd.MetricSpectrum(dens, vectors=True)
    spec.update(x)
    after = cmf_amd.MetricStatistics(dens)
    macs_after = after.update(x)
    assert torch.equal(before.state.flat, after.state.flat) and torch.equal(macs_before, macs_after)
    for coordinates in ("noise",):
        a, b = cmf_amd.MetricStatistics(dens, coordinates=coordinates), cmf_amd.MetricStatistics(dens, coordinates=coordinates)
        a.update(x), cmf_amd.MetricSpectrum(dens, coordinates=coordinates).update(x), b.update(x)
        assert torch.equal(a.state.flat, b.state.flat)
