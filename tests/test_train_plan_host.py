"""``engine.resnet_coupler_plan`` on the CPU: the plans of named couplers written out by hand, and every plan against the launches
``net_primal``, ``net_cotangent`` and ``net_primal_backward`` then make (recorded by tests/_launch_trace.py, no kernel runs).  The
traces equal tests/golden/train_trace.json, recorded by ``tests/dev/train_trace.py --tree <worktree> --golden`` from commit 734194a, the
parent of the commit that introduced the plan: the passes make the launches they made when each decided inline.  The full matrix and
the comparison with another checkout: tests/dev/train_trace.py."""
import json
import os

import pytest

import _launch_trace as LT
from cmf_amd import engine as E

P = E.CouplerPlan
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_trace.json")
DEFAULT, TIP = LT.CONFIGS[0], "train-if-possible"


def _plan(shape, hid, B, nc, need_acts, config=DEFAULT, nb=1, view="checkerboard"):
    H, W, cin, cout = shape
    net = LT._resnet(cin, nb, cout, hid)
    with E.scope(E.KernelConfig(tangent=config[0], primal=config[1])):
        return E.resnet_coupler_plan(net, LT.net_view(E, H, W, cin, E._resnet_parts(net)[0].out_channels, view), B, nc, need_acts)


@pytest.fixture(scope="module")
def cases():
    """label -> dict(kw, plan, passes): every row of the subset planned and traced once under the same KernelConfig."""
    out = {}
    for label, kw in LT.train_subset():
        plan = _plan((kw["H"], kw["W"], kw["cin"], kw["cout"]), kw["hid"], kw["B"], kw["nc"], kw["need_acts"],
                     (kw["tangent"], kw["primal"]), kw["nb"], kw["view"])
        assert label not in out
        out[label] = dict(kw=kw, plan=plan, passes=LT.run_train(E, **kw))
    assert len(out) <= 500 and set(out) <= {label for label, _ in LT.train_matrix()}
    return out


def test_the_subset_reaches_every_value_of_every_field(cases):
    plans = [c["plan"] for c in cases.values()]
    assert all(isinstance(p, P) for p in plans)
    for field in ("grouped", "masks", "split", "wgrad_bits", "batched", "bwd16"):
        assert {type(getattr(p, field)) for p in plans} == {bool} and {getattr(p, field) for p in plans} == {True, False}, field
    assert {p.arith for p in plans} == {"f16x3", "f32", "bf16x3"} and {p.multiple for p in plans} == {16, 32}
    assert {repr(p.acts) for p in plans} == {"False", "True", "'bits'", "'train'"}


def test_expected_plans():
    #                                                      grouped arith  masks  acts  split wgrad_bits multiple batched bwd16
    # the MNIST checkerboard coupler 1 -> 64 -> 2 at 28 x 28 under the default KernelConfig, a sweep of 64 column slots
    for B in (32, 64):
        assert _plan(LT.MNIST, 64, B, 64, TIP) == (True, "f16x3", True, "train", True, True, 32, True, True)
        assert _plan(LT.MNIST, 64, B, 64, "sweep") == (True, "f16x3", True, "bits", True, True, 32, True, True)
        assert _plan(LT.MNIST, 64, B, 64, False) == (True, "f16x3", False, False, True, True, 32, True, True)
    # whole groups of 16 but not of 32: grouped floats, nothing to train from; B = 8: per-sample convs, the backward pads to 32
    assert _plan(LT.MNIST, 64, 16, 64, TIP) == (True, "f16x3", False, True, True, True, 32, True, True)
    assert _plan(LT.MNIST, 64, 8, 64, TIP) == (False, "f16x3", False, True, True, True, 32, True, True)
    assert _plan(LT.MNIST, 64, 8, 64, "sweep") == (False, "f16x3", False, True, True, True, 32, True, True)
    # 16 column slots: the weight gradients read floats, so no ActList; a primal-only pass (no sweep yet) hands one out
    assert _plan(LT.MNIST, 64, 32, 16, TIP) == (True, "f16x3", False, True, True, False, 32, True, True)
    assert _plan(LT.MNIST, 64, 32, None, TIP) == (True, "f16x3", True, "train", True, False, 32, True, True)
    # each primal arithmetic: exact fp32 writes masks too, the bf16 split kernel writes none
    assert _plan(LT.MNIST, 64, 32, 64, TIP, ("bf16x3", "f32")) == (True, "f32", True, "train", True, True, 32, True, False)
    assert _plan(LT.MNIST, 64, 32, 64, TIP, ("bf16x3", "bf16x3")) == (True, "bf16x3", False, True, True, True, 32, True, False)
    assert _plan(LT.MNIST, 64, 32, 64, "bits", ("bf16x3", "bf16x3")) == (True, "bf16x3", False, True, True, True, 32, True, False)
    assert _plan(LT.MNIST, 64, 32, 64, "train", ("bf16x3", "bf16x3")) == (True, "bf16x3", False, "train", True, True, 32, True, False)
    # exact-fp32 tangents: fp32 reverse sweep on floats, groups of 16 in the backward, one weight gradient per launch
    assert _plan(LT.MNIST, 64, 32, 64, TIP, ("f32", "f16x3")) == (True, "f16x3", False, True, False, False, 16, False, True)
    assert _plan(LT.MNIST, 64, 32, 64, "sweep", ("f32", "f16x3")) == (True, "f16x3", False, True, False, False, 16, False, True)
    assert _plan(LT.MNIST, 64, 32, None, TIP, ("f32", "f32")) == (True, "f32", True, "train", False, False, 16, False, False)
    # hid 128: the split primal kernels do not take the width (fp32 forward; the backward form carries no bias and does), the hidden
    # weight gradients go out one by one.  hid 32: one 32-channel group is the bf16 split kernel's alone
    assert _plan(LT.HALF, 128, 32, 32, TIP) == (True, "f32", True, "train", True, True, 32, False, True)
    assert _plan(LT.HALF, 128, 32, 32, TIP, ("bf16x3", "bf16x3")) == (True, "f32", False, True, True, True, 32, False, False)
    assert _plan(LT.HALF, 32, 32, 32, TIP) == (True, "f32", False, True, False, False, 16, False, False)
    assert _plan(LT.HALF, 32, 32, 32, "bits") == (True, "f32", True, "bits", False, False, 16, False, False)
    assert _plan(LT.HALF, 32, 32, 32, TIP, ("bf16x3", "bf16x3")) == (True, "bf16x3", False, True, False, False, 16, False, False)
    # 7 x 7: no pixel tiling of the split kernels -- per-sample primal, fp32 sweep; the weight gradients still pair the groups
    assert _plan(LT.ODD, 64, 32, 32, TIP) == (False, "f16x3", False, True, False, False, 32, True, False)
    # the batched weight gradients stop where one problem fills the chip: 256 image rows (9 paired groups of 28 rows: 252)
    assert _plan(LT.MNIST, 64, 288, 64, TIP).batched and not _plan(LT.MNIST, 64, 320, 64, TIP).batched


def test_train_acts_mode_reads_the_plan():
    """On every coupler, batch, sweep width and KernelConfig of the matrix ``train_acts_mode`` is the plan's answer to
    "train-if-possible", and that is the rule it held before the plan: groups of 32, the split kernel's shapes in whole 64-channel
    groups, a primal arithmetic that writes masks and -- when the sweep's width is known -- split weight gradients on column pairs."""
    n = 0
    for (shape, hid), B, nc, config in LT.itertools.product(LT.TRAIN_NETS, LT.TRAIN_B, (None,) + LT.TRAIN_NC, LT.CONFIGS):
        H, W, cin, cout = shape
        net, view = LT._resnet(cin, 1, cout, hid), LT.net_view(E, H, W, cin, hid, "checkerboard")
        want = (B % 32 == 0 and config[1] != "bf16x3" and hid % 64 == 0 and (W % 14 == 0 and H % 2 == 0 or W % 8 == 0 and H % 4 == 0)
                and (nc is None or (config[0] == "bf16x3" and nc % 32 == 0)))
        with E.scope(E.KernelConfig(tangent=config[0], primal=config[1])):
            got = E.train_acts_mode(net, view, B, nc=nc)
            assert got == ("train" if want else True) == E.resnet_coupler_plan(net, view, B, nc, TIP).acts, (shape, hid, B, nc, config)
            if nc is not None:
                assert E.train_acts_mode(net, view, B, E.Tangent(B, view.geom.N, nc, "panel", "cpu")) == got
        n += got == "train"
    assert n > 20 and E.train_acts_mode(LT.mlp_case(E)["net"], LT.mlp_case(E)["view"], 32) is True


def test_the_traces_equal_the_recorded_ones(cases):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert set(golden) == set(cases)
    got = {label: {p: LT.digest(r) for p, r in c["passes"].items()} for label, c in cases.items()}
    assert {label: d for label, d in got.items() if d != golden[label]} == {}


def _launches(c, p, name):
    return [(a, dict(k)) for n, a, k in c["passes"].get(p, ((), None))[0] if n == name]


def test_the_launches_are_what_the_plan_says(cases):
    for label, c in cases.items():
        p, kw = c["plan"], c["kw"]
        nb, hid = kw["nb"], kw["hid"] if kw["nb"] else kw["cout"]
        prim = [k for a, k in _launches(c, "primal", "conv_tangent")]
        acts = c["passes"]["primal"][1][2]
        assert (len(prim) == 2 * nb) == p.grouped or nb == 0, label
        assert bool(_launches(c, "primal", "primal_regroup")) == p.grouped, label
        assert all(k["precision"] == p.arith and ("mask_out" in k) == p.masks for k in prim), label
        assert len(_launches(c, "primal", "absmax")) == (p.grouped and p.arith == "f16x3"), label
        # what came back: nothing, an ActList, or a list whose hidden elements but the last are BitMasks exactly under "bits"
        if p.grouped:
            form = False if acts is None else "train" if acts[0] == "ActList" else \
                "bits" if nb and all(a[0] == "BitMask" for a in acts[1:-1]) else True
            assert form == p.acts or (nb == 0 and p.acts == "bits"), label
            if form == "train":
                assert all((a[0] == "BitMask") == p.masks for a in acts[1][1:-1]) and len(acts[2]) == 2 * nb + 1, label
        # reverse sweep: the hidden transposed convs take relu' as an output bit mask on the split kernel, floats in fp32
        hidden = [k for a, k in _launches(c, "cotangent", "conv_tangent") if a[6] == 9 and a[12] == a[13] == hid]
        assert all((k["fo"][0] == "BitMask") == p.split and (k.get("precision") == "f32") != p.split for k in hidden), label
        wg = [(a, k) for a, k in _launches(c, "cotangent", "conv_tangent_wgrad") if a[11] == 9 and a[13] == a[14] == hid]
        assert all((k["f"][0] == "BitMask") == p.wgrad_bits for a, k in wg), label
        if "backward" in c["passes"]:
            groups = {a[0].split(":")[1] for a, k in _launches(c, "backward", "primal_regroup") if a[1] is True}
            assert all(int(g.strip("()").split(",")[0]) % p.multiple == 0 for g in groups) and groups, label
            assert bool(_launches(c, "backward", "conv_tangent_wgrad_batched")) == (p.batched and nb > 0), label
            assert bool(_launches(c, "backward", "channel_sum_batched")) == (p.batched and nb > 0), label
            bwd = [k for a, k in _launches(c, "backward", "conv_tangent") if a[6] == 9 and a[12] == a[13] == hid]
            assert len(bwd) == 2 * nb and all((k["precision"] == "f16x3") == p.bwd16 for k in bwd), label
            assert len(_launches(c, "backward", "absmax")) == p.bwd16, label


def test_invariants_read_off_the_traces(cases):
    """What used to be held together by asserts on the device, read off the launches alone."""
    trained = batched = ranged = 0
    for label, c in cases.items():
        p, kw = c["plan"], c["kw"]
        hid = kw["hid"] if kw["nb"] else kw["cout"]
        for name in c["passes"]:
            for a, k in _launches(c, name, "conv_tangent"):
                if k.get("precision") == "f16x3":                    # the fp16 split kernel never runs without its range words
                    assert k.get("amax_in") is not None and k.get("amax_out") is not None, label
                    ranged += 1
            for a, k in _launches(c, name, "conv_tangent_wgrad"):
                if isinstance(k.get("f"), tuple) and k["f"][0] == "BitMask":
                    assert a[11] == 9 and a[13] % 64 == 0 and a[14] % 64 == 0 and a[17] % 32 == 0, label
        if p.acts == "train" and "cotangent" in c["passes"]:         # an ActList is only handed to a split reverse sweep
            hidden = [k for a, k in _launches(c, "cotangent", "conv_tangent") if a[6] == 9 and a[12] == a[13] == hid]
            assert all(k["fo"][0] == "BitMask" and "precision" not in k for k in hidden) and (hidden or not kw["nb"]), label
            trained += 1
        if "backward" in c["passes"] and kw["nb"]:
            assert bool(_launches(c, "backward", "conv_tangent_wgrad_batched")) == p.batched, label
            batched += p.batched
    assert trained > 5 and batched > 5 and ranged > 50
