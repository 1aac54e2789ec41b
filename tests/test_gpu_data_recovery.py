"""``cmf_amd.ManifoldProjector.recover(..., space="data")`` on the GPU: linear inverse problems whose operator acts
on pixel values, behind the logit wrapper, end to end on ``mini_mnist`` through the DENSITY (dequantise, scalar-mult, scalar-add,
logit, head) under the conditions tests/test_data_recovery_host.py establishes on the float64 reference loop; the identity chain of
the tabular fixtures; sub-batches; and what must stay as it was.  Needs an MI355X: run with ``-m gpu``."""
import pytest
import torch

import _data_recovery_reference as DR
import _recovery_reference as RR
from test_gpu_metric_stats import build
from test_gpu_recovery import KEYS, known_answer_problem, run_recover

pytestmark = pytest.mark.gpu


def run_data(dens, head, y, A, steps, **start):
    """One ``recover(space="data")`` with ``run_recover``'s side-effect and shape checks."""
    return run_recover(dens, head, y, A, steps, space="data", **start)


def wrapper_of(dens, head):
    """(wa, wc, logit) of the fixture's density, as the projector reduces its chain."""
    from cmf_amd.projection import data_space_wrapper, wrapper_bijections
    wa, wc, logit, perm = data_space_wrapper(wrapper_bijections(dens, head))
    assert perm is None
    return wa, wc, logit


@pytest.fixture(scope="module")
def problem():
    """The fixture and, per operator kind, (u_on, A, y, x_start) on the GPU: u_on the float64 data-space image of the GPU's own
    g(z_0) at the encoder's latent of the fixture's input (on the host), y = A u_on formed in float64 on the host, and the data-
    space input the recovery starts from.  Computed once; nothing below modifies it."""
    g, meta, dens, head, x = build(DR.NAME)
    x = x[:DR.BATCH].contiguous()
    with torch.no_grad():
        z0 = dens.extract_latent(x.clone(), earliest_latent=False)
        x_on = head.flow_forward(z0)
    wa, wc, logit = wrapper_of(dens, head)
    assert logit
    dm = DR.DataModel(None, (wa, wc, logit))
    u_on = dm.wrapper(x_on.cpu().double())[0]
    x_start = DR.start_input(dm, x_on.cpu()).float().cuda().contiguous()
    cases = {}
    for kind in DR.DATA_E2E_TOL:
        A = DR.operator(kind)                                         # on the CPU, the product of the builders included
        cases[kind] = (A.cuda().contiguous(), RR.measure(A, u_on).float().cuda().contiguous())
    return g, dens, head, x, u_on, x_start, cases


@pytest.mark.parametrize("kind", list(DR.DATA_E2E_TOL))
def test_recovery_finds_the_known_answer(kind, problem):
    """y = A u(g(z_0)): ten steps from the encoder's latent of the perturbed input must reconstruct u_on over all D pixel values
    within ``DR.DATA_E2E_TOL``, for every sample.  "gaussian": the seeded Gaussian operator, M = 32; "built": downsample(2) of a
    3 x 3 box blur from ``cmf_amd.operators``, M = 196."""
    from cmf_amd import engine as E
    g, dens, head, x, u_on, x_start, cases = problem
    A, y = cases[kind]
    assert A.shape == ({"gaussian": DR.M_GAUSSIAN, "built": 196}[kind], 784)
    _, out = run_data(dens, head, y, A, 10, x_init=x_start)
    rel = DR.rel_distance(out["reconstruction"], u_on)
    start = DR.rel_distance(x_start, u_on)
    print(f"{DR.NAME}, {kind}: M = {A.shape[0]}: ||u - u_on|| / ||u_on|| <= {float(rel.max()):.3e} (tolerance "
          f"{DR.DATA_E2E_TOL[kind]:.3e}; the start is off by {float(start.min()):.3e} .. {float(start.max()):.3e}); cost "
          f"{float(out['initial_cost'].max()):.3e} -> {float(out['cost'].max()):.3e}; accepted {out['accepted'].tolist()}")
    assert out["reconstruction"].shape == x.shape
    assert bool((rel <= DR.DATA_E2E_TOL[kind]).all())
    assert bool((out["cost"] <= out["initial_cost"]).all()) and bool((out["info"] == 0).all())
    with torch.no_grad():
        assert torch.equal(out["reconstruction_head"], head.flow_forward(out["latent"]))
    w = wrapper_of(dens, head)
    assert torch.equal(out["measurement"], E.operator_image_wrapped(A, out["reconstruction_head"], w))
    assert torch.equal(out["cost"], E.residual_sqnorm(y, out["measurement"])[0])


@pytest.mark.parametrize("name", ["c2a_power", "c2b_hepmass"])
def test_identity_chain_gives_the_head_space_bits(name):
    """No wrapper in front of the head: the triple is (1, 0, 0), u is x_hat and s is 1, so every key is ``space="head"``'s."""
    g, meta, dens, head, x = build(name)
    assert wrapper_of(dens, head) == (1.0, 0.0, False)
    x_on, A, y, x_start = known_answer_problem(name, head, dens, x)
    _, data = run_data(dens, head, y, A, 10, x_init=x_start)
    _, ref = run_recover(dens, head, y, A, 10, x_init=x_start)
    assert bool((ref["accepted"] > 0).any()) and bool((ref["info"] == 0).all())
    for key in KEYS:
        assert torch.equal(data[key], ref[key]), key


def test_sub_batches_give_the_rows_of_one_call(problem, monkeypatch):
    """B = 3 as 2 + 1, under the conditions of test_gpu_recovery.py's test of the same name."""
    from cmf_amd import engine as E
    g, dens, head, x, u_on, x_start, cases = problem
    A, y = cases["gaussian"]
    _, whole = run_data(dens, head, y, A, 10, x_init=x_start)
    prog = head.program
    monkeypatch.setattr(prog, "TANGENT_BUDGET", 2 * prog.tangent_bytes_per_sample(E.ceil16(prog.d)))
    assert prog.tangent_chunk(3) == 2                              # B = 3 runs as sub-batches of 2 and 1
    _, pieces = run_data(dens, head, y, A, 10, x_init=x_start)
    c0 = whole["initial_cost"]
    print(f"pieces against whole: bit-equal latent {torch.equal(pieces['latent'], whole['latent'])}, cost / initial cost "
          f"{float((pieces['cost'] / c0).max()):.2e} against {float((whole['cost'] / c0).max()):.2e}")
    assert float(((pieces["initial_cost"] - c0).abs() / c0).max()) <= 1e-5
    assert float(((pieces["cost"] - whole["cost"]).abs() / c0).max()) <= 1e-5
    assert bool((DR.rel_distance(pieces["reconstruction"], u_on) <= DR.DATA_E2E_TOL["gaussian"]).all())
    assert bool((pieces["info"] == 0).all()) and bool((whole["info"] == 0).all())


def test_the_log_density_path_is_untouched(problem):
    """``run_recover`` holds the inputs and ``head.last_gram`` to what they were; elbo before and after is bit-equal."""
    g, dens, head, x, u_on, x_start, cases = problem
    raw = g["x"].float().cuda()                                      # elbo dequantises its input itself: the seeded noise below
    A, y = cases["built"]
    with torch.no_grad():
        torch.manual_seed(11)
        elbo_before = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
        _, out = run_data(dens, head, y, A, 3, x_init=x_start)
        torch.manual_seed(11)
        elbo_after = dens.elbo(raw.clone(), add_reconstruction=True)["elbo"]
    assert bool(torch.isfinite(elbo_before).all()) and torch.equal(elbo_before, elbo_after)
    assert bool((out["info"] == 0).all())


def test_head_space_recovery_keeps_its_bits(problem):
    """``recover`` without ``space`` on test_gpu_recovery.py's mini_mnist known-answer case: the same bits before and after a
    ``space="data"`` call in the same process, and ``space="head"`` is that default."""
    g, dens, head, x, u_on, x_start, cases = problem
    x_on, A, y, h_start = known_answer_problem(DR.NAME, head, dens, x)
    _, before = run_recover(head, head, y, A, 10, x_init=h_start)
    run_data(dens, head, cases["gaussian"][1], cases["gaussian"][0], 10, x_init=x_start)
    _, after = run_recover(head, head, y, A, 10, x_init=h_start)
    _, named = run_recover(head, head, y, A, 10, x_init=h_start, space="head")
    assert bool((RR.rel_distance(before["reconstruction_head"], x_on) <= RR.E2E_TOL[DR.NAME]).all())
    for key in KEYS:
        assert torch.equal(before[key], after[key]) and torch.equal(before[key], named[key]), key


def test_space_is_checked_on_the_gpu_too(problem):
    g, dens, head, x, u_on, x_start, cases = problem
    import cmf_amd
    A, y = cases["gaussian"]
    with pytest.raises(ValueError, match="space must be 'head' or 'data'"):
        cmf_amd.ManifoldProjector(dens).recover(y, A, x_init=x_start, space="pixels")
