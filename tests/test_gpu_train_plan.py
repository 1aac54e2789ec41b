"""The CPU launch traces of a training step through one ResNet coupler (tests/_launch_trace.py ``run_train``) tell the truth on the
device: one coupler, 14 x 14, 2 -> 64 -> 4 with one block, nc = 32, at B = 8, 16 and 32 under the default KernelConfig and under exact
fp32, runs the real ``net_primal`` -> ``net_tangent(save=[])`` -> ``net_cotangent(saved, grads)`` -> ``net_primal_backward``.  The timer
family names of the launches (they carry ``_primal``, ``_primal_bwd`` and ``_batched``) are the ones the CPU trace of the same case
derives, and every gradient and the two input cotangents have the bits recorded in tests/golden/train_plan_bits.json by
tests/dev/record_train_plan_bits.py on an MI355X from commit 734194a (the parent of the commit that planned these passes in
``engine.resnet_coupler_plan``), where two recordings agreed bit for bit on every tensor (``not_reproducible`` is empty)."""
import collections
import hashlib
import json
import os

import pytest
import torch

import _launch_trace as LT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_plan_bits.json")
SHAPE, HID, NB, NC, VIEW = LT.HALF, 64, 1, 32, "checkerboard"
CASES = [(B, config) for config in (("bf16x3", "f16x3"), ("f32", "f32")) for B in (8, 16, 32)]
label = lambda B, config: f"B={B} tangent={config[0]} primal={config[1]}"


def _inputs(B):
    """The coupler with every parameter drawn from one CPU generator, its view, and the step's inputs -- all on the device."""
    from cmf_amd import engine as E, networks
    H, W, cin, cout = SHAPE
    gen = torch.Generator().manual_seed(7100)
    net = networks.get_resnet(cin, [HID] * NB, cout)
    with torch.no_grad():
        for p in net.parameters():
            fan = p[0].numel() if p.dim() == 4 else 1
            p.copy_(torch.randn(p.shape, generator=gen) * (fan ** -0.5 if p.dim() == 4 else 0.1) + (1.0 if p is net.weights else 0.0))
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    view = LT.net_view(E, H, W, cin, HID, VIEW)
    view.mask, view.live, view.probe = view.mask.cuda(), None, None
    return dict(net=net.cuda(), view=view, z=rnd(B, cin, H, W), v=rnd(B, cin * H * W, NC), yc=rnd(B, cout * H * W, NC),
                dy=rnd(B, cout, H, W), dg=rnd(B, cout, H, W))


def run(B, config):
    """-> (timer family names in launch order, {tensor name: SHA-1 of its bytes}, {tensor name: the tensor on the CPU})."""
    from cmf_amd import engine as E
    c = _inputs(B)
    net, view, z = c["net"], c["view"], c["z"]
    with E.scope(E.KernelConfig(tangent=config[0], primal=config[1])), E.timing(lambda n: True) as timer, torch.no_grad():
        y, g, acts = E.net_primal(net, z, view, need_acts=E.train_acts_mode(net, view, B, nc=NC))
        saved, grads = [], {}
        E.net_tangent(net, E.Tangent.from_dense(c["v"], NC, "panel"), view, acts, save=saved)
        Ct = E.Tangent.from_dense(torch.zeros_like(c["v"]), NC, "panel")
        E.net_cotangent(net, E.Tangent.from_dense(c["yc"], NC, "panel"), view, acts, Ct, saved=saved, grads=grads)
        dz = torch.zeros_like(z)
        E.net_primal_backward(net, z, view, acts, y, g, c["dy"], c["dg"], grads, dz)
        torch.cuda.synchronize()
    out = {n: grads[p].cpu() for n, p in net.named_parameters()}
    out.update(dz=dz.cpu(), ct=Ct.to_dense(NC).contiguous().cpu())
    sha = {n: hashlib.sha1(t.contiguous().numpy().tobytes()).hexdigest() for n, t in out.items()}
    return [r[0] for r in timer.records], sha, out


def take_record():
    """What tests/dev/record_train_plan_bits.py writes: the digests of one run per case."""
    return {label(B, config): run(B, config)[1] for B, config in CASES}


@pytest.mark.parametrize("B,config", CASES, ids=[label(*c).replace(" ", "-") for c in CASES])
def test_the_traced_launches_run_and_give_the_recorded_bits(B, config):
    from cmf_amd import engine as E
    with open(GOLDEN) as f:
        golden = json.load(f)
    H, W, cin, cout = SHAPE
    traced = LT.run_train(E, H, W, cin, cout, HID, NB, B, NC, VIEW, *config, need_acts="train-if-possible", training=True)
    want = collections.Counter(n for p in ("primal", "tangent", "cotangent", "backward") for n in LT.families(E, traced[p][0]))
    names, sha, out = run(B, config)
    print(f"train_plan {label(B, config)}: {len(names)} timed launches, {dict(collections.Counter(names))}")
    assert collections.Counter(names) == want
    assert any(n.endswith("_primal_bwd") for n in names) and any("_primal" in n and "wgrad" in n for n in names)
    loose = golden["not_reproducible"].get(label(B, config), [])
    assert not loose, "a tensor the recording commit does not reproduce needs its values in the golden file, at the gradient tolerance " \
                      "of test_training_from_grouped_activations_and_bit_masks_gives_the_same_gradients"
    rec = golden["cases"][label(B, config)]
    assert set(sha) == set(rec) and all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in out.values())
    assert {n: d for n, d in sha.items() if d != rec[n]} == {}
