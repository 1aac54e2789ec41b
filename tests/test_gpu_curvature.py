"""``cmf_amd.ManifoldCurvature`` on the GPU against the float64 reference pipeline (tests/_curvature_reference.py) at the
same latents, the same frames and the same step -- so rounding is compared, not truncation --, under the conditions
tests/test_curvature_host.py establishes.  Needs an MI355X: run with ``-m gpu``.

Allowance (the rule of DESIGN 4.3h): a tensor may deviate from the float64 reference by max(1e-4, 3 x the float32 oracle's own deviation)
of the tensor's largest magnitude, all in the max-norm over the fixture's batch.  ``sectional`` is compared on the planes whose
reference numerator R_abab and denominator g_aa g_bb - g_ab^2 are both above their allowances (dnum = the allowance of ``riemann``, dden =
the allowance of ``frame_metric`` times g_aa + g_bb + 2 |g_ab|), within (dnum + |K| dden) / (den - dden); the planes are selected from
the reference alone and at least half of them must qualify.  ``asymmetry``: the batch's largest against 10 x the float32 oracle's."""
import pytest
import torch

import _curvature_reference as CR
from cmf_amd.curvature import ManifoldCurvature
from test_gpu_metric_stats import build

pytestmark = pytest.mark.gpu

STEP = ManifoldCurvature.DEFAULT_STEP
CASES = [("c1_sphere_d2", 2), ("c2a_power", 2), ("c2b_hepmass", 2), ("c2b_hepmass", 4)]
KEYS = ("frame", "step", "frame_metric", "second_gram", "christoffel", "riemann", "sectional", "scalar", "normal_curvature", "asymmetry",
        "cancellation", "info")

_BUILT = {}


def built(name):
    if name not in _BUILT:
        _BUILT[name] = build(name)
    return _BUILT[name]


def curvature_of(name, step=None):
    import cmf_amd
    _, _, dens, head, x = built(name)
    return cmf_amd.ManifoldCurvature(dens, step=step), dens, head, x


def run_at_latents(name, z, frame, step=None):
    """One ``at_latents`` with the side-effect and shape checks every case makes; the result on the CPU."""
    curv, _, head, _ = curvature_of(name)
    marker = object()
    head.last_gram = marker
    zc, keep = z.cuda(), z.clone()
    out = curv.at_latents(zc, None if frame is None else frame.cuda(), step)
    torch.cuda.synchronize()
    assert head.last_gram is marker and torch.equal(zc.cpu(), keep)
    B, d = z.shape
    m = min(d, 4) if frame is None else frame.shape[-1]
    q = m * (m + 1) // 2
    shapes = {"frame": (B, d, m), "step": (B,), "frame_metric": (B, m, m), "second_gram": (B, q, q), "christoffel": (B, q, d),
              "riemann": (B, m, m, m, m), "sectional": (B, m, m), "scalar": (B,), "normal_curvature": (B, m), "asymmetry": (B,),
              "cancellation": (B,), "info": (B,)}
    assert set(out) == set(KEYS)
    for k, v in out.items():
        assert tuple(v.shape) == shapes[k] and v.dtype == (torch.int32 if k == "info" else torch.float64) and v.is_cuda, k
    return {k: v.cpu() for k, v in out.items()}


def symmetries_hold(Rm, scale):
    assert torch.equal(Rm, -Rm.transpose(1, 2)) and torch.equal(Rm, -Rm.transpose(3, 4)) and torch.equal(Rm, Rm.permute(0, 3, 4, 1, 2))
    bianchi = Rm + Rm.permute(0, 1, 3, 4, 2) + Rm.permute(0, 1, 4, 2, 3)
    assert float(bianchi.abs().max()) <= 8 * 2.0 ** -53 * scale


@pytest.mark.parametrize("name,m", CASES)
def test_mlp_fixtures_match_the_float64_reference(name, m):
    z, frame, ref = CR.run(name, m, STEP)
    _, _, o32 = CR.run(name, m, STEP, torch.float32)
    out = run_at_latents(name, z, frame, STEP)
    assert bool((out["info"] == 0).all()) and bool((out["step"] == STEP).all())
    assert float((out["frame"] - frame).abs().max()) <= 4 * 2.0 ** -53          # unit columns, normalised once more
    tol = {}
    for key in ("second_gram", "christoffel", "riemann", "frame_metric", "normal_curvature"):
        yard = CR.deviation(o32[key], ref[key])
        tol[key] = max(1e-4, 3.0 * yard)
        dev = CR.deviation(out[key], ref[key])
        print(f"{name} m={m} {key}: deviation {dev:.2e}, float32 oracle {yard:.2e}, allowance {tol[key]:.2e}")
        assert dev <= tol[key], key
    symmetries_hold(out["riemann"], float(out["second_gram"].abs().max()))
    # sectional curvature, on the planes the reference can resolve
    g, Rr, K = ref["frame_metric"], ref["riemann"], ref["sectional"]
    ar = torch.arange(m)
    diag = g[:, ar, ar]
    den = diag[:, :, None] * diag[:, None, :] - g * g
    num = Rr[:, ar[:, None], ar[None, :], ar[:, None], ar[None, :]]
    dnum = tol["riemann"] * float(Rr.abs().max())
    dden = tol["frame_metric"] * float(g.abs().max()) * (diag[:, :, None] + diag[:, None, :] + 2.0 * g.abs())
    off = ~torch.eye(m, dtype=torch.bool)[None].expand_as(K)
    ok = off & (num.abs() > dnum) & (den > dden)
    share = float(ok.sum()) / float(off.sum())
    bound = (dnum + K.abs() * dden) / (den - dden).clamp_min(1e-300)
    err = (out["sectional"] - K).abs()
    print(f"{name} m={m} sectional: {int(ok.sum())} of {int(off.sum())} planes qualify, worst error / bound "
          f"{float((err / bound)[ok].max()):.3f}, worst relative error {float((err / K.abs())[ok].max()):.2e}")
    assert share >= 0.5 and bool((err[ok] <= bound[ok]).all())
    assert bool((out["sectional"][:, ar, ar] == 0).all())
    a_max, a32 = float(out["asymmetry"].max()), float(o32["asymmetry"].max())
    print(f"{name} m={m} asymmetry: {a_max:.2e}, float32 oracle {a32:.2e}, float64 reference {float(ref['asymmetry'].max()):.2e}; "
          f"cancellation min {float(out['cancellation'].min()):.2e}")
    assert a_max <= 10.0 * a32
    if z.shape[1] == 2 and m == 2:
        assert float((out["scalar"] - 2.0 * out["sectional"][:, 0, 1]).abs().max()) <= 1e-12 * float(out["scalar"].abs().max())


@pytest.mark.parametrize("m", [2, 4])
def test_relu_fixture_is_flagged(m):
    z, frame, ref = CR.run("mini_mnist", m, STEP, seed=CR.RELU_SEED)
    out = run_at_latents("mini_mnist", z, frame, STEP)
    assert bool((out["info"] == 0).all())
    assert all(bool(torch.isfinite(out[k]).all()) for k in KEYS if k != "info")
    print(f"mini_mnist m={m}: asymmetry {[round(float(a), 3) for a in out['asymmetry']]}, reference "
          f"{[round(float(a), 3) for a in ref['asymmetry']]}")
    flagged = ref["asymmetry"] >= 0.5
    assert bool(flagged.any()) and bool((out["asymmetry"][flagged] > 0.1).all())


def test_full_size_mnist_sample():
    """The only fixture that reaches the bf16x3 kernels and the 28 x 28 plans: shapes, finiteness and ``info``; the deviation from the
    float32 oracle at the same step is printed (DESIGN 4.3m records it), without a threshold."""
    z, frame, o32 = CR.run("c3_mnist_full", 2, STEP, torch.float32, samples=(0,))
    out = run_at_latents("c3_mnist_full", z, frame, STEP)
    assert bool((out["info"] == 0).all())
    assert all(bool(torch.isfinite(out[k]).all()) for k in KEYS if k != "info")
    for key in ("second_gram", "christoffel", "frame_metric", "normal_curvature"):
        print(f"c3_mnist_full m=2 {key}: deviation from the float32 oracle {CR.deviation(out[key], o32[key]):.2e}")
    print(f"c3_mnist_full m=2 asymmetry {float(out['asymmetry'][0]):.3f}, float32 oracle {float(o32['asymmetry'][0]):.3f}")


def test_sub_batches_default_frame_shared_frame_and_inputs(monkeypatch):
    from cmf_amd import engine as E
    name, m = "c2b_hepmass", 2
    z, frame, _ = CR.run(name, m, STEP)
    curv, dens, head, x = curvature_of(name)
    prog = head.program
    B, d = z.shape
    whole = run_at_latents(name, z, frame)
    assert bool((whole["step"] == curv.DEFAULT_STEP).all())
    # the default frame is the axis frame; a shared frame is its broadcast
    axes = torch.eye(d, min(d, 4), dtype=torch.float64)
    default, explicit = run_at_latents(name, z, None), run_at_latents(name, z, axes.expand(B, -1, -1).contiguous())
    shared, spread = run_at_latents(name, z, frame[0]), run_at_latents(name, z, frame[:1].expand(B, -1, -1).contiguous())
    for key in KEYS:
        assert torch.equal(default[key], explicit[key]) and torch.equal(shared[key], spread[key]), key
    # float32 directions of any length give the same normalised frame to rounding
    scaled = run_at_latents(name, z, (3.0 * frame).float())
    assert float((scaled["frame"] - frame).abs().max()) <= 2.0 ** -23
    # at(x) is at_latents at the projector's latent, by bits; x is not modified
    keep, marker = x.clone(), object()
    head.last_gram = marker
    with torch.no_grad(), E.scope(head.kernels):
        zp = curv.projector.head_input_and_latent(x)[1]
    by_x, by_z = curv.at(x, frame.cuda()), curv.at_latents(zp, frame.cuda())
    torch.cuda.synchronize()
    assert head.last_gram is marker and torch.equal(x, keep)
    for key in KEYS:
        assert torch.equal(by_x[key], by_z[key]), key
    # sub-batches of whole samples
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * (2 * m + 1) * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert 1 <= prog.tangent_chunk(B * (2 * m + 1)) // (2 * m + 1) < B
    pieces = run_at_latents(name, z, frame)
    for key in KEYS:
        assert torch.equal(pieces[key], whole[key]), key
    monkeypatch.setattr(prog, "TANGENT_BUDGET", prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    with pytest.raises(ValueError, match="directions"):
        curv.at_latents(z.cuda(), frame.cuda())


def test_failed_samples_are_nan_and_confined(monkeypatch):
    """``info`` 2 from a NaN latent and ``info`` 1 from a metric that is singular as the kernel sees it (the real ``gram_cholesky`` of
    the real sweep with row and column 1 of one sample's Gram matrix zeroed on its way to the kernel): which outputs are NaN and which
    are kept, ``asymmetry`` above all -- a gate on its maximum must not pass over a failed sample --, and every other sample by bits."""
    from cmf_amd import engine as E
    name, m = "c2b_hepmass", 2
    z, frame, _ = CR.run(name, m, STEP)
    curv, _, head, _ = curvature_of(name)
    B = z.shape[0]
    assert B >= 3
    clean = run_at_latents(name, z, frame)
    assert bool((clean["info"] == 0).all()) and bool((clean["asymmetry"] > 0).all())
    bad = z.clone()
    bad[1, 0] = float("nan")
    real = E.gram_cholesky

    def singular(T, d, *args, **kwargs):
        r = real(T, d, *args, **kwargs)
        r.jtj[2, 1, :] = 0.0
        r.jtj[2, :, 1] = 0.0
        return r

    monkeypatch.setattr(E, "gram_cholesky", singular)
    out = curv.at_latents(bad.cuda(), frame.cuda())
    torch.cuda.synchronize()
    monkeypatch.undo()
    out = {k: v.cpu() for k, v in out.items()}
    assert out["info"].tolist() == [0, 2, 1] + [0] * (B - 3)
    results = [k for k in KEYS if k not in ("frame", "step", "info")]
    for k in results:
        assert bool(torch.isnan(out[k][1]).all()), k                         # code 2: every result of the sample
    for k in results:
        if k in ("frame_metric", "asymmetry"):                               # code 1: what does not need G^-1 is kept
            assert bool(torch.isfinite(out[k][2]).all()), k
        else:
            assert bool(torch.isnan(out[k][2]).all()), k
    assert torch.equal(out["asymmetry"][2], clean["asymmetry"][2])
    assert not float(out["asymmetry"].max()) < 1.0                           # the gate a user would write sees the failed sample
    assert torch.equal(out["frame"], clean["frame"]) and torch.equal(out["step"], clean["step"])
    for b in [0] + list(range(3, B)):
        for k in KEYS:
            assert torch.equal(out[k][b], clean[k][b]), (b, k)


def test_refusals(monkeypatch):
    import cmf_amd
    name = "c2b_hepmass"
    curv, dens, head, x = curvature_of(name)
    z = CR.latents(name).cuda()
    B, d = z.shape
    good = torch.eye(d, 2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="1 <= m"):
        curv.at_latents(z, torch.eye(d, 5, dtype=torch.float64, device="cuda"))                # m > 4
    zero = good.clone()
    zero[:, 1] = 0.0
    with pytest.raises(ValueError, match="finite and not zero"):
        curv.at_latents(z, zero)
    bad = good.clone()
    bad[0, 0] = float("nan")
    with pytest.raises(ValueError, match="finite and not zero"):
        curv.at_latents(z, bad)
    with pytest.raises(ValueError, match="GPU"):
        curv.at_latents(z.cpu(), good)
    with pytest.raises(ValueError, match="GPU"):
        curv.at_latents(z, good.cpu())
    with pytest.raises(ValueError, match="GPU"):
        curv.at(x.cpu())
    with pytest.raises(ValueError, match="directions must be"):
        curv.at_latents(z, torch.eye(d + 1, 2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="directions must be"):
        curv.at_latents(z, torch.ones(d, 2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="float32"):
        curv.at_latents(z.double(), good)
    for step in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="step"):
            curv.at_latents(z, good, step)
        with pytest.raises(ValueError, match="step"):
            cmf_amd.ManifoldCurvature(dens, step=step)
    # m > d on the two-dimensional fixture
    c2, _, _, _ = curvature_of("c1_sphere_d2")
    z2 = CR.latents("c1_sphere_d2").cuda()
    with pytest.raises(ValueError, match="1 <= m"):
        c2.at_latents(z2, torch.ones(2, 3, dtype=torch.float64, device="cuda"))
    # d > 128 at construction
    monkeypatch.setattr(head.program, "d", 129)
    with pytest.raises(ValueError, match="latent_dimension = 129"):
        cmf_amd.ManifoldCurvature(dens)
    monkeypatch.undo()
