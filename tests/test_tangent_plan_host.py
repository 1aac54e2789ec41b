"""``engine.resnet_tangent_plan`` on the CPU: the plans of named couplers written out by hand, what each switch changes, and every plan
against the launches ``engine.net_tangent`` then makes (recorded by tests/_launch_trace.py, no kernel runs).  The full matrix and the
comparison with another checkout: tests/dev/net_tangent_trace.py."""
import itertools

import pytest

import _launch_trace as LT
from cmf_amd import engine as E

P = E.TangentPlan
MNIST, HALF, ODD = (28, 28, 1, 2), (14, 14, 2, 4), (7, 7, 8, 16)


def _rows():
    """(key, case keywords, save, tangent, switch off): every switch position on two shapes, the other axes with all switches on."""
    def row(shape, nb, size, view, bits, save=None, tangent="bf16x3", off=None, grouped=False):
        kw = dict(zip(("H", "W", "cin", "cout"), shape), nb=nb, nc=size[0], B=size[1], view=view, bits=bits, grouped=grouped)
        return (shape, nb, size[0], view, bits, grouped, save is not None, tangent, off), kw, save, tangent, off
    for shape, sizes in ((MNIST, LT.SIZES), (HALF, LT.SIZES[1:])):
        for nb, size, view, bits, off in itertools.product((1, 2), sizes, LT.VIEWS, (True, False), (None,) + LT.SWITCHES):
            yield row(shape, nb, size, view, bits, off=off)
    for shape, view, (save, tangent) in itertools.product((MNIST, HALF), LT.VIEWS, (([], "bf16x3"), (None, "f32"), ([], "f32"))):
        yield row(shape, 2, LT.SIZES[2], view, True, save=save, tangent=tangent)
    for view in LT.VIEWS:
        yield row(MNIST, 0, LT.SIZES[2], view, True)
        yield row(MNIST, 3, LT.SIZES[2], view, True)
        yield row(ODD, 2, LT.SIZES[2], view, True)
        yield row(MNIST, 2, LT.SIZES[2], view, False, grouped=True)


@pytest.fixture(scope="module")
def cases():
    """key -> dict(kw, plan, launches, shape, compact), planned and traced once under the same switches and KernelConfig."""
    out = {}
    for key, kw, save, tangent, off in _rows():
        c = LT.resnet_case(E, **kw)
        with LT.switched_off(E, off), E.scope(E.KernelConfig(tangent=tangent)):
            plan = E.resnet_tangent_plan(c["net"], c["view"], kw["nc"], c["T"].layout, c["acts"], save is not None)
        with LT.switched_off(E, off):
            launches, shape, compact = LT.trace(E, **c, save=None if save is None else [], tangent=tangent)
        assert key not in out
        out[key] = dict(kw=kw, plan=plan, launches=launches, shape=shape, compact=compact)
    assert len(out) <= 500
    return out


def _plan(cases, shape, nb, nc, view, bits=True, grouped=False, save=False, tangent="bf16x3", off=None):
    return cases[(shape, nb, nc, view, bits, grouped, save, tangent, off)]["plan"]


def test_the_subset_reaches_every_plan_value_and_every_switch(cases):
    plans = [c["plan"] for c in cases.values()]
    assert {p.front for p in plans} == {"plain", "probe", "seeded"}
    assert {p.tail for p in plans} == {"plain", "live", "head", "block"}
    assert {p.filt for p in plans} == {True, False} and {p.compact for p in plans} == {True, False}
    for sw in LT.SWITCHES:                               # each switch is off somewhere, and being off changes a plan there
        assert any(k[-1] == sw and c["plan"] != cases[k[:-1] + (None,)]["plan"] for k, c in cases.items()), sw
    assert all(isinstance(p, P) and type(p.filt) is bool and type(p.compact) is bool for p in plans)


def test_expected_plans(cases):
    plan = lambda *a, **k: tuple(_plan(cases, *a, **k))
    # the 28 x 28 checkerboard coupler 1 -> 64 -> 2 on bit masks, 64 column slots: two blocks, one block, three blocks
    assert plan(MNIST, 2, 64, "checkerboard") == (True, "seeded", "block", True)
    assert plan(MNIST, 1, 64, "checkerboard") == (True, "probe", "head", True)
    assert plan(MNIST, 3, 64, "checkerboard") == (True, "seeded", "block", True)
    assert plan(MNIST, 2, 32, "checkerboard") == (True, "seeded", "block", True)
    # nc = 16 does not exceed the plan's one slice of probe columns: no probe front
    assert plan(MNIST, 2, 16, "checkerboard") == (True, "plain", "block", True)
    assert plan(MNIST, 1, 16, "checkerboard") == (True, "plain", "head", True)
    # 14 x 14 checkerboard, 2 -> 64 -> 4: neither shape set holds it
    assert plan(HALF, 2, 64, "checkerboard") == (True, "plain", "head", True)
    assert plan(HALF, 1, 64, "checkerboard") == (True, "plain", "head", True)
    # split-channel couplers (no ``live``, no mask) keep their launches; a mask and a probe plan without ``live`` keep the tail
    assert plan(MNIST, 2, 64, "split") == (True, "plain", "plain", False)
    assert plan(HALF, 2, 64, "split") == (True, "plain", "plain", False)
    assert plan(MNIST, 2, 64, "mask") == (True, "seeded", "plain", False)
    # float activations: no folded launch and no seeding (both read bit masks); the probe front and the live tail do not
    assert plan(MNIST, 2, 64, "checkerboard", bits=False) == (True, "probe", "live", True)
    assert plan(HALF, 2, 64, "checkerboard", bits=False) == (True, "plain", "live", True)
    assert plan(MNIST, 2, 64, "checkerboard", bits=False, grouped=True) == (True, "plain", "plain", False)
    # no block; a width the split kernel does not take; training; exact-fp32 tangents
    assert plan(MNIST, 0, 64, "checkerboard") == (False, "plain", "plain", False)        # hid = cout = 2: not the split kernel
    assert plan(ODD, 2, 64, "checkerboard") == (False, "plain", "plain", False)
    for view in LT.VIEWS:
        for shape in (MNIST, HALF):
            assert plan(shape, 2, 64, view, save=True) == (False, "plain", "plain", False)
            assert plan(shape, 2, 64, view, tangent="f32") == (False, "plain", "plain", False)
            assert plan(shape, 2, 64, view, save=True, tangent="f32") == (False, "plain", "plain", False)


def test_a_switch_changes_only_what_it_gates(cases):
    """With one switch off the plan is the all-on plan with that form absent -- every other field as it was."""
    without = {
        "CHECKERBOARD_TAIL": lambda p: p._replace(compact=False, tail="plain" if p.tail == "live" else p.tail),
        "SKIP_DEAD_ROWS": lambda p: p._replace(filt=False),
        "FOLD_HEAD": lambda p: p._replace(tail="live" if p.tail in ("head", "block") else p.tail),     # CHECKERBOARD_TAIL holds here
        "FOLD_BLOCK": lambda p: p._replace(tail="head" if p.tail == "block" else p.tail),
        "PROBE_FRONT": lambda p: p._replace(front="plain"),
        "SEED_RESIDUAL": lambda p: p._replace(front="probe" if p.front == "seeded" else p.front),
    }
    n = 0
    for key, c in cases.items():
        if key[-1] is not None:
            assert c["plan"] == without[key[-1]](cases[key[:-1] + (None,)]["plan"]), key
            n += 1
    assert n == 6 * sum(k[:-1] + ("FOLD_HEAD",) in cases for k in cases if k[-1] is None) and n > 300


def test_the_launches_are_what_the_plan_says(cases):
    for key, c in cases.items():
        p, kw, names = c["plan"], c["kw"], [l[0] for l in c["launches"]]
        convs = [(a, dict(k)) for name, a, k in c["launches"] if name == "conv_tangent"]
        nb, HW = kw["nb"], kw["H"] * kw["W"]
        assert ("probe_apply" in names) == (p.front != "plain"), key
        assert names.count("probe_apply") == names.count("_probe_hidden") == (p.front != "plain"), key
        assert names.count("seed_panel") == names.count("_seed_pack") == (p.front == "seeded"), key
        # the thin first conv: the one 3 x 3 launch without a relu' factor (F_RAW under a mask, F_NONE without one)
        thin = [k for a, k in convs if a[6] == 9 and k["fmode"] in (E.F_RAW, E.F_NONE)]
        assert len(thin) == (p.front != "seeded"), key
        assert all(k["fmode"] == (E.F_NONE if kw["view"] == "split" else E.F_RAW) for k in thin), key
        heads = [dict(k["head"]) for a, k in convs if k.get("head") is not None]
        assert len(heads) == (p.tail in ("head", "block")), key
        assert all(("conv1" in h) == (p.tail == "block") for h in heads), key
        assert names.count("gather_primal") == (p.tail == "live"), key
        # conv1 launches (the probe front's response launch included) are the ones that name a store filter
        conv1 = [k for a, k in convs if "ymask" in k]
        c1_bits = kw["bits"] and not kw["grouped"]
        assert len(conv1) == nb - (p.tail == "block"), key
        assert all((k["ymask"] is not None) == (p.filt and c1_bits) for k in conv1), key
        applies = [dict(k) for name, a, k in c["launches"] if name == "probe_apply"]
        assert all((k["ymask"] is not None) == (p.filt and c1_bits) for k in applies), key
        assert c["compact"] == p.compact, key
        assert c["shape"] == (kw["B"], kw["cout"] * (HW // 2 if p.compact else HW), kw["nc"], "panel"), key
        assert len(convs) == (p.front != "seeded") + 2 * nb - (p.tail == "block") + (p.tail in ("plain", "live")), key


def test_compact_is_a_declared_attribute_of_tangent():
    t = E.Tangent(1, 4, 16, "panel", "cpu")
    assert t.compact is False and E.Tangent(1, 4, 16, "panel", "cpu", compact=True).compact is True
