"""The host side of the head and manifold wrappers of ``cmf_amd.engine`` on the CPU, no kernel runs: (a) what each wrapper refuses
and in which words, (b) the timer entry -- family name, flops, bytes -- each reports, both against the record
tests/golden/engine_wrappers_host.json taken at commit ec77635 by tests/dev/record_engine_wrappers.py, before the argument rules and
the timer dispatch were each given one definition; (c) ``projection.lm_loop`` against a plain per-row Python model.

The refusals all happen before any launch, so a tensor that merely says it is on the GPU reaches every rule; for the timer entries a
stub timer records what ``wrap`` is handed and does not launch."""
import contextlib
import json
import math
import os

import pytest
import torch

from cmf_amd import engine as E
from cmf_amd import projection
from cmf_amd.projection import DAMPING_MAX, DAMPING_MIN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_wrappers_host.json")
F32, F64 = torch.float32, torch.float64


class FakeGpu(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True."""

    @property
    def is_cuda(self):
        return True


class OtherGpu(FakeGpu):
    """... and names another device than its neighbours."""

    @property
    def device(self):
        return torch.device("cuda", 1)


def gpu(*shape, dtype=F32, cls=FakeGpu):
    return torch.zeros(*shape, dtype=dtype).as_subclass(cls)


def tangent(B, N, nc, data=None):
    return E.Tangent(B, N, nc, "panel", "cpu", data=gpu(B * N * nc) if data is None else data)


def strided(*shape, dtype=F32):
    """A non-contiguous tensor of ``shape`` (every second element of the last dimension of a wider one)."""
    return gpu(*shape[:-1], 2 * shape[-1], dtype=dtype)[..., ::2]


def tensor_faults(shape, dtype=F32):
    """The faults every tensor argument can have on its own, by name; the other dtype stands in for the wrong one."""
    return {"not_a_tensor": [[0.0]], "cpu": torch.zeros(*shape, dtype=dtype),
            "dtype": gpu(*shape, dtype=F64 if dtype == F32 else F32), "not_contiguous": strided(*shape, dtype=dtype)}


def gram_faults(rows, d):
    """... and those of a Gram stack (rows, d, d) beside them (the width limits are cases of their own: other arguments follow d)."""
    return dict(tensor_faults((rows, d, d)), rank=gpu(rows, d), not_square=gpu(rows, d, d + 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# well-formed arguments of every wrapper, as keywords; a case replaces some of them
# ---------------------------------------------------------------------------------------------------------------------------------
B, D, N = 2, 3, 5                                   # samples, latent width, elements per sample
CURVES, POINTS = 2, 4                               # curve_step / curve_energy / cross_gram
T_POINTS, M = 3, 2                                  # transport_chain


def spectrum_args(d=D):
    return dict(jtj=gpu(B, d, d))


def residual_args():
    return dict(x=gpu(B, N), xhat=gpu(B, N))


def gn_args(d=D, nc=16):
    return dict(T=tangent(B, N, nc), jtj=gpu(B, d, d), x=gpu(B, N), xhat=gpu(B, N), damping=gpu(B, dtype=F64))


def cross_gram_args(d=D, nc=16, points=POINTS):
    return dict(T=tangent(CURVES * POINTS, N, nc), d=d, points=points)


def energy_args():
    return dict(xhat=gpu(CURVES * POINTS, N), points=POINTS)


def curve_step_args(d=D, nc=16):
    rows = CURVES * POINTS
    return dict(T=tangent(rows, N, nc), jtj=gpu(rows, d, d), cross=gpu(CURVES, POINTS - 3, d, d), xhat=gpu(rows, N), points=POINTS,
                damping=gpu(CURVES, dtype=F64))


def solve_args(d=D):
    return dict(jtj=gpu(B, d, d), rhs=gpu(B, d, dtype=F64))


def transport_args(d=D, m=M):
    rows = CURVES * T_POINTS
    return dict(jtj=gpu(rows, d, d), cross=gpu(rows - 1, d, d), w0=gpu(CURVES, m, d, dtype=F64), points=T_POINTS)


def _refusals():
    """id -> (wrapper, keywords): every call breaks exactly one rule, or has one tensor on the CPU / on another GPU."""
    out = {}

    def add(fn, base, arg, faults):
        for what, value in faults.items():
            out[f"{fn.__name__}:{arg}:{what}"] = (fn, {**base(), arg: value})

    def damping_faults(rows):
        return {"not_a_tensor": 1e-3, "dtype": gpu(rows), "shape": gpu(rows + 1, dtype=F64), "not_contiguous": strided(rows, dtype=F64),
                "device": gpu(rows, dtype=F64, cls=OtherGpu)}

    def pair_faults(rows):
        return dict(tensor_faults((rows, N)), rank=gpu(rows))

    # gram_spectrum
    add(E.gram_spectrum, spectrum_args, "jtj", gram_faults(B, D))
    for d in (0, 129):
        out[f"gram_spectrum:d={d}"] = (E.gram_spectrum, spectrum_args(d))
    # residual_sqnorm
    for arg in ("x", "xhat"):
        add(E.residual_sqnorm, residual_args, arg, pair_faults(B))
    add(E.residual_sqnorm, residual_args, "xhat", {"shape": gpu(B, N + 1), "device": gpu(B, N, cls=OtherGpu)})
    out["residual_sqnorm:no_elements"] = (E.residual_sqnorm, dict(x=gpu(B, 0), xhat=gpu(B, 0)))
    # gauss_newton_step
    add(E.gauss_newton_step, gn_args, "T", {"not_a_tangent": gpu(B, N, 16)})
    for arg in ("x", "xhat"):
        add(E.gauss_newton_step, gn_args, arg, pair_faults(B))
    add(E.gauss_newton_step, gn_args, "xhat", {"shape": gpu(B, N + 1), "device": gpu(B, N, cls=OtherGpu)})
    add(E.gauss_newton_step, gn_args, "jtj", dict(gram_faults(B, D), rows=gpu(B + 1, D, D), device=gpu(B, D, D, cls=OtherGpu)))
    for d in (0, 129):
        out[f"gauss_newton_step:d={d}"] = (E.gauss_newton_step, gn_args(d, nc=16 if d == 0 else 144))
    add(E.gauss_newton_step, gn_args, "T", {
        "samples": tangent(B + 1, N, 16), "elements": tangent(B, N + 1, 16), "nc_not_16": tangent(B, N, 8),
        "device": tangent(B, N, 16, gpu(B * N * 16, cls=OtherGpu))})
    out["gauss_newton_step:T:nc_below_d"] = (E.gauss_newton_step, gn_args(d=17))
    add(E.gauss_newton_step, gn_args, "damping", damping_faults(B))
    # cross_gram
    add(E.cross_gram, cross_gram_args, "T", {
        "not_a_tangent": gpu(CURVES * POINTS, N, 16), "cpu": tangent(CURVES * POINTS, N, 16, torch.zeros(CURVES * POINTS * N * 16)),
        "nc_not_16": tangent(CURVES * POINTS, N, 8), "nc_above_128": tangent(CURVES * POINTS, N, 144),
        "not_whole_curves": tangent(CURVES * POINTS + 1, N, 16)})
    out["cross_gram:T:nc_below_d"] = (E.cross_gram, cross_gram_args(d=17))
    for d in (0, 129):
        out[f"cross_gram:d={d}"] = (E.cross_gram, cross_gram_args(d, nc=16 if d == 0 else 144))
    out["cross_gram:points=2"] = (E.cross_gram, cross_gram_args(points=2))
    # curve_energy
    add(E.curve_energy, energy_args, "xhat", dict(pair_faults(CURVES * POINTS), not_whole_curves=gpu(CURVES * POINTS + 1, N),
                                                  no_elements=gpu(CURVES * POINTS, 0)))
    add(E.curve_energy, energy_args, "points", {"2": 2})
    # curve_step
    rows = CURVES * POINTS
    add(E.curve_step, curve_step_args, "xhat", dict(pair_faults(rows), device=gpu(rows, N, cls=OtherGpu),
                                                    no_elements=gpu(rows, 0), elements=gpu(rows, N + 1)))
    add(E.curve_step, curve_step_args, "jtj", dict(gram_faults(rows, D), rows=gpu(rows + POINTS, D, D),
                                                   device=gpu(rows, D, D, cls=OtherGpu)))
    for d in (0, 129):
        out[f"curve_step:d={d}"] = (E.curve_step, curve_step_args(d, nc=16 if d == 0 else 144))
    add(E.curve_step, curve_step_args, "cross", dict(tensor_faults((CURVES, POINTS - 3, D, D)), shape=gpu(CURVES, POINTS - 2, D, D),
                                                     device=gpu(CURVES, POINTS - 3, D, D, cls=OtherGpu)))
    add(E.curve_step, curve_step_args, "T", {
        "not_a_tangent": gpu(rows, N, 16), "cpu": tangent(rows, N, 16, torch.zeros(rows * N * 16)), "nc_not_16": tangent(rows, N, 8),
        "nc_above_128": tangent(rows, N, 144), "not_whole_curves": tangent(rows + 1, N, 16), "curves": tangent(rows + POINTS, N, 16),
        "elements": tangent(rows, N + 1, 16), "device": tangent(rows, N, 16, gpu(rows * N * 16, cls=OtherGpu))})
    out["curve_step:T:nc_below_d"] = (E.curve_step, curve_step_args(d=17))
    out["curve_step:points=2"] = (E.curve_step, {**curve_step_args(), "points": 2})
    out["curve_step:points=3"] = (E.curve_step, {**curve_step_args(), "points": 3})          # 8 samples are no whole curves of 3
    add(E.curve_step, curve_step_args, "damping", damping_faults(CURVES))
    # metric_solve
    add(E.metric_solve, solve_args, "jtj", gram_faults(B, D))
    for d in (0, 129):
        out[f"metric_solve:d={d}"] = (E.metric_solve, solve_args(d))
    add(E.metric_solve, solve_args, "rhs", dict(tensor_faults((B, D), F64), shape=gpu(B, D + 1, dtype=F64), rank=gpu(B, D, 1, dtype=F64),
                                                device=gpu(B, D, dtype=F64, cls=OtherGpu)))
    # transport_chain
    rows = CURVES * T_POINTS
    add(E.transport_chain, transport_args, "jtj", gram_faults(rows, D))
    for d in (0, 129):
        out[f"transport_chain:d={d}"] = (E.transport_chain, transport_args(d))
    out["transport_chain:points=1"] = (E.transport_chain, {**transport_args(), "points": 1, "w0": gpu(rows, M, D, dtype=F64)})
    out["transport_chain:points=4"] = (E.transport_chain, {**transport_args(), "points": 4})  # 6 samples are no whole curves of 4
    add(E.transport_chain, transport_args, "w0", dict(
        tensor_faults((CURVES, M, D), F64), rank=gpu(CURVES, D, dtype=F64), curves=gpu(CURVES + 1, M, D, dtype=F64),
        width=gpu(CURVES, M, D + 1, dtype=F64), device=gpu(CURVES, M, D, dtype=F64, cls=OtherGpu)))
    for m in (0, 17):
        out[f"transport_chain:m={m}"] = (E.transport_chain, transport_args(m=m))
    add(E.transport_chain, transport_args, "cross", dict(tensor_faults((rows - 1, D, D)), shape=gpu(rows, D, D),
                                                         device=gpu(rows - 1, D, D, cls=OtherGpu)))
    return out


REFUSALS = _refusals()

#: id -> (wrapper, keywords) of one small well-formed call each (and the variants whose cost formula differs)
TIMED = {
    "gram_spectrum": (E.gram_spectrum, spectrum_args()),
    "gram_spectrum:vectors": (E.gram_spectrum, dict(spectrum_args(), vectors=True)),
    "residual_sqnorm": (E.residual_sqnorm, residual_args()),
    "gauss_newton_step": (E.gauss_newton_step, gn_args()),
    "gauss_newton_step:d=17,nc=32": (E.gauss_newton_step, gn_args(17, 32)),
    "cross_gram": (E.cross_gram, cross_gram_args()),
    "curve_energy": (E.curve_energy, energy_args()),
    "curve_step": (E.curve_step, curve_step_args()),
    "metric_solve": (E.metric_solve, solve_args()),
    "metric_solve:apply": (E.metric_solve, dict(solve_args(), apply=True)),
    "transport_chain": (E.transport_chain, transport_args()),
}


class StubTimer:
    """Records what ``wrap`` is handed and launches nothing."""

    def __init__(self):
        self.records = []

    def wrap(self, name, flops, nbytes, launch):
        self.records.append((name, flops, nbytes))


class StubLibrary:
    """What ``curve_step`` asks the library before its launch: a workspace size."""

    @staticmethod
    def cmf_curve_step_ws(d, points, curves):
        return 64


@contextlib.contextmanager
def stub_library():
    load, E._lib.load = E._lib.load, StubLibrary
    try:
        yield
    finally:
        E._lib.load = load


def refusal(case):
    """[exception type, message] of a call of ``REFUSALS``, or None when it is not refused."""
    fn, kw = REFUSALS[case]
    try:
        with stub_library():
            fn(**kw)
    except Exception as e:                          # noqa: BLE001  (the type is part of what is compared)
        return [type(e).__name__, str(e)]
    return None


def timer_entries(case):
    """The [name, flops, bytes] entries a call of ``TIMED`` reports to the timer of its thread."""
    fn, kw = TIMED[case]
    stub = StubTimer()
    with E._use_timer(stub), stub_library():
        fn(**kw)
    return [list(r) for r in stub.records]


def take_record():
    """What tests/dev/record_engine_wrappers.py writes."""
    return {"refusals": {case: refusal(case) for case in REFUSALS}, "timer": {case: timer_entries(case) for case in TIMED}}


@pytest.fixture(scope="module")
def record():
    with open(GOLDEN) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_record_covers_the_tables(record):
    assert set(record["refusals"]) == set(REFUSALS) and set(record["timer"]) == set(TIMED)
    assert all(r is not None and r[0] == "ValueError" for r in record["refusals"].values())


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_type_and_message(record, case):
    assert case in record["refusals"], f"no record for {case}"
    assert refusal(case) == record["refusals"][case]


def test_refusals_cover_every_rule(record):
    """Every argument rule of the eight wrappers is the one that fires in some case: the table reaches them all."""
    messages = " | ".join(r[1] for r in record["refusals"].values())
    for words in ("must be on the GPU", "must be float32", "must be float64", "(not contiguous)", "must be an engine.Tangent",
                  "the spectrum kernel supports", "the Gauss-Newton step kernel supports", "the curve kernels support",
                  "the metric solve kernel supports", "the transport kernel supports", "a curve needs points >= 3",
                  "a curve needs points >= 2", "samples of xhat must be whole curves", "samples of T must be whole curves",
                  "samples of jtj must be whole curves", "at least one element per sample", "at least one element per point",
                  "must agree", "for the 2 samples of 5 elements of x", "for the 8 samples of 5 elements of xhat",
                  "nc <= 128 columns", "damping must be 2 contiguous float64 values", "vectors per launch", "on cuda:1",
                  "rhs must be a contiguous (2, 3) tensor on", "w0 must be a contiguous (2, m, 3) tensor on",
                  "cross must be a contiguous (5, 3, 3) tensor on", "cross must be a contiguous (2, 1, 3, 3) tensor,"):
        assert words in messages, words


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) timer entries
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(TIMED))
def test_timer_entry(record, case):
    assert case in record["timer"], f"no record for {case}"
    got = timer_entries(case)
    assert len(got) == 1 and got == record["timer"][case]


def _counter():
    calls = []
    return calls, lambda: calls.append(1) or "launched"


def test_timed_without_a_timer_launches_once_and_never_costs():
    calls, launch = _counter()

    def cost():
        raise AssertionError("the cost of a launch is evaluated only for a timer")
    assert E._timer() is None
    assert E._timed("family", cost, launch) == "launched" and len(calls) == 1


def test_timed_without_a_name_launches_once_and_records_nothing():
    calls, launch = _counter()
    stub = StubTimer()
    with E._use_timer(stub):
        assert E._timed(None, lambda: (1.0, 2.0), launch) == "launched"
    assert len(calls) == 1 and stub.records == []


def test_timed_hands_the_launch_to_the_timer():
    calls, launch = _counter()
    stub = StubTimer()
    with E._use_timer(stub):
        E._timed("family", lambda: (1.0, 2.0), launch)
    assert stub.records == [("family", 1.0, 2.0)] and calls == []      # the timer launches, and the stub does not
    timer = E.KernelTimer(lambda name: False)                           # a family the timer does not select: a plain launch
    with E._use_timer(timer):
        assert E._timed("family", lambda: (1.0, 2.0), launch) == "launched"
    assert len(calls) == 1 and timer.records == []


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the accept/reject loop against a per-row model
# ---------------------------------------------------------------------------------------------------------------------------------
LOWER, EQUAL, NAN, UNSOLVED = "solved and lower", "solved and equal", "solved and NaN", "not solved"
#: SCRIPT[step][row]: the four outcomes row by row in the first step, then mixed so that rows accept after rejecting and back
SCRIPT = ((LOWER, EQUAL, NAN, UNSOLVED),
          (LOWER, LOWER, UNSOLVED, NAN),
          (LOWER, EQUAL, LOWER, UNSOLVED))
UP, DOWN = 10.0, 0.1
LAM0 = (1e-11, 1e7, 1.0, 1e7)                       # row 0 is held at DAMPING_MIN from its second step on, row 3 at DAMPING_MAX
COST0 = (8.0, 4.0, 2.0, 1.0)


def _proposal(kind, step, z, cost):
    """What the scripted trial proposes to a row: (solved, new z, new cost)."""
    new_cost = {LOWER: cost / 2, EQUAL: cost, NAN: math.nan, UNSOLVED: cost / 2}[kind]
    return kind != UNSOLVED, z + (step + 1), new_cost


def _model(steps):
    """The loop for one row at a time in plain Python: per row (z, cost, lam, accepted, the lam each trial saw)."""
    rows = []
    for row in range(4):
        z, cost, lam, accepted, seen = float(row), COST0[row], LAM0[row], 0, []
        for step in range(steps):
            seen.append(lam)
            solved, z_new, cost_new = _proposal(SCRIPT[step][row], step, z, cost)
            if solved and cost_new < cost:
                z, cost, lam, accepted = z_new, cost_new, max(lam * DOWN, DAMPING_MIN), accepted + 1
            else:
                lam = min(lam * UP, DAMPING_MAX)
        rows.append((z, cost, lam, accepted, seen))
    return rows


@pytest.mark.parametrize("steps", (0, 3))
def test_lm_loop_against_a_per_row_model(steps):
    z0 = torch.arange(4, dtype=F32)[:, None, None].expand(4, 2, 3).contiguous()          # a state entry of rank 3
    state0 = (z0, z0[:, 0, 0].double().clone(), torch.tensor(COST0, dtype=F64))           # ... of rank 1, and the cost
    seen, step = [], [0]

    def trial(state, lam):
        seen.append(lam.tolist())
        z, _, cost = state
        rows = [_proposal(SCRIPT[step[0]][row], step[0], float(z[row, 0, 0]), float(cost[row])) for row in range(4)]
        step[0] += 1
        z_new = torch.tensor([r[1] for r in rows], dtype=F32)[:, None, None].expand(4, 2, 3).contiguous()
        return torch.tensor([r[0] for r in rows]), (z_new, z_new[:, 0, 0].double(), torch.tensor([r[2] for r in rows], dtype=F64))

    (z, zd, cost), lam, accepted = projection.lm_loop(state0, 2, torch.tensor(LAM0, dtype=F64), steps, UP, DOWN, trial)
    model = _model(steps)
    assert step[0] == steps and accepted.dtype == torch.int32 and lam.dtype == F64
    for row, (z_row, cost_row, lam_row, accepted_row, seen_row) in enumerate(model):
        assert z[row].tolist() == [[z_row] * 3] * 2 and zd[row].item() == z_row
        assert cost[row].item() == cost_row and lam[row].item() == lam_row and accepted[row].item() == accepted_row
        assert [s[row] for s in seen] == seen_row
    if steps == 3:                                  # the script does what it is for: every outcome, both clamps, a NaN never taken
        assert [m[3] for m in model] == [3, 1, 1, 0]
        assert model[0][4][-1] == model[0][2] == DAMPING_MIN and model[3][4][-1] == model[3][2] == DAMPING_MAX
        assert not torch.isnan(cost).any()
