"""CPU checks of tests/_mlp_coupler_elements.py: the mirror of cmf_mlp_coupler's dispatch is pinned to the launcher's source lines
and puts every GPU case on the kernel its name says; the fp32 emulation of the kernels' summation order stays within the asserted
constants with the factor four to spare and within the float64 model's per-element bound, on every case's own inputs; the bound is
small against the values it guards; ``pack_image`` is the layout the kernel's header describes."""
import math

import numpy as np
import pytest
import torch

import _mlp_coupler_elements as M

CUS = 256                                                                  # the CU count the emulation's batches are sized for
_ids = [c.id for c in M.CASES]


def test_dispatch_rules_are_the_ones_mirrored():
    """``variant`` restates the shape rules of cmf_mlp_coupler and its launchers; the lines must still be in the source."""
    assert M.missing_dispatch_lines() == []


@pytest.mark.parametrize("cus", [256, 304, 64])
@pytest.mark.parametrize("case", M.CASES, ids=_ids)
def test_every_case_reaches_the_path_its_name_says(case, cus):
    v = case.variant(cus)
    assert v.path == case.want_path, (case.id, cus, v)
    assert v.lds <= 160 * 1024
    if "percu2" in case.id:
        assert v.per_cu == 2 and v.n_tiles > 2 * cus == v.grid, v
    elif case.want_path[3]:
        assert v.per_cu == 1 and v.n_tiles > cus == v.grid, v
    if "dead-waves" in case.id:
        assert v.n_tiles == 1 and case.B(cus) < v.NW * v.spt
    if "ragged" in case.id or "pack" in case.id:
        assert case.B(cus) % (v.NW * v.spt if v.kernel != "split" else 16) != 0
    if case.tangent:                                                       # the PRIMAL-mode decode of the same inputs
        assert case.variant(cus, None).kernel == ("split" if v.HT == 8 else "primal")


def test_the_cases_cover_the_launch_paths():
    paths = {c.want_path for c in M.CASES}
    assert paths >= {("tangent", 1, 4, False), ("tangent", 2, 8, False), ("tangent", 2, 8, True), ("tangent", 8, 4, True), ("tangent", 8, 8, True),
                     ("tangent", 8, 4, False), ("primal", 1, 8, False), ("primal", 2, 8, True), ("primal", 8, 8, True),
                     ("split", 8, 8, False), ("split", 8, 8, True)}
    assert {c.ncols for c in M.CASES if c.id.startswith("tan-ht1-nw4-pack")} == {2, 3, 4, 5, 7, 8}
    assert {len(c.hidden) % 2 for c in M.CASES if c.want_path == ("split", 8, 8, True)} == {0, 1}     # odd and even layer counts
    offs = {(c.pass_idx[0] != 0, (c.pass_idx[1] - c.pass_idx[0]) if len(c.pass_idx) > 1 else 1) for c in M.CASES}
    assert {o[0] for o in offs} == {False, True} and {o[1] for o in offs} == {1, 2}
    assert {c.weights for c in M.CASES if len(c.hidden) > 1 and min(c.hidden) > 32} == {"sparse"}
    assert all(c.weights == "dense" for c in M.CASES if len(c.hidden) == 1 or max(c.hidden) <= 32)


@pytest.mark.parametrize("case", M.CASES, ids=_ids)
def test_emulation_meets_the_bound(case):
    """The fp32 emulation in the kernels' order, per dot product and end to end, and the size of the bound itself."""
    d = M.case_data(case, CUS)
    for mode in case.modes:
        kern, ref = M.kernel_of(case, CUS, mode), d.ref[mode]
        e = M.emulate(case, d, mode, kern)
        print(f"\nMLP_COUPLER_HOST {case.id} {mode} [{kern}]: dot error 2^{math.log2(e.dot_ratio):.2f} of |W||h| + |b| "
              f"(C_DOT 2^{math.log2(M.C_DOT[kern]):.0f}), {e.dot_ceiling:.3f} of the rigorous (K + 1) u; median bound / |want| = "
              f"{M.bound_over_value(ref, case):.1e}; s in [{float(ref.s.min()):.1f}, {float(ref.s.max()):.1f}]")
        assert 4 * e.dot_ratio <= M.C_DOT[kern], (case.id, mode, math.log2(e.dot_ratio))
        assert e.dot_ceiling <= 1.0, (case.id, mode, e.dot_ceiling)
        M.check_elements(f"emulation {case.id} {mode}", ref, e.z, e.T, e.lj, idx=e.idx, tag="MLP_COUPLER_HOST")
        assert M.bound_over_value(ref, case) < 1e-3, (case.id, mode)           # or the bound would pass anything
    if case.tangent:
        ref = d.ref["tangent"]
        assert float(ref.s.min()) < -2 and float(ref.s.max()) > 2 or d.B < 8, "s spans about +-3"
        assert bool((ref.T_bound[:, case.pass_idx] == 0).all()) and bool((ref.T_bound[:, case.mod_idx] > 0).all())
    h0 = torch.tanh(d.z[:, case.pass_idx].double() @ d.net[0][0].double().T + d.net[0][1].double())[:, ::7]
    assert float((1 - h0 * h0).median()) < 2.0 ** -12, "every seventh first-layer unit is saturated"


def test_c_dot_is_four_times_the_emulation_rounded_up():
    worst = {k: 0.0 for k in M.C_DOT}
    for case in M.CASES:
        d = M.case_data(case, CUS)
        for mode in case.modes:
            kern = M.kernel_of(case, CUS, mode)
            worst[kern] = max(worst[kern], M.emulate(case, d, mode, kern).dot_ratio)
    for kern, w in worst.items():
        print(f"\nMLP_COUPLER_HOST largest emulated dot error [{kern}] 2^{math.log2(w):.2f}; C_DOT 2^{math.log2(M.C_DOT[kern]):.0f}")
        assert M.C_DOT[kern] == 2.0 ** math.ceil(math.log2(4 * w)), (kern, math.log2(w))
    assert (M.C_TANH, M.C_EXP) == (5.0, 3.0)


@pytest.mark.parametrize("case", [c for c in M.CASES if c.tangent], ids=[c.id for c in M.CASES if c.tangent])
def test_column_scales_pass_through_the_emulation_bit_for_bit(case):
    """emulate(graded columns) == emulate(unit columns) 2^-(3 j): powers of two commute with every operation on a column."""
    d = M.case_data(case, CUS)
    g = M.emulate(case, d, "tangent", M.kernel_of(case, CUS, "tangent"))
    u = M.Data()
    u.__dict__.update(d.__dict__)
    u.V = d.Vu
    un = M.emulate(case, u, "tangent", M.kernel_of(case, CUS, "tangent"))
    assert torch.equal(g.T, un.T * M.column_scales(case.ncols)) and torch.equal(g.z, un.z)


# ---------------------------------------------------------------------------------------------------------------------------
# pack_image
PACK_SHAPES = [(10, 3, 1, 1), (10, 3, 2, 1), (33, 21, 3, 2), (33, 21, 8, 2), (128, 128, 8, 8), (64, 128, 4, 8), (10, 10, 1, 1), (4, 10, 1, 2),
               (17, 32, 2, 2), (22, 128, 2, 8)]


@pytest.mark.parametrize("out_f,in_f,n_mt,n_kg", PACK_SHAPES)
@pytest.mark.parametrize("first", [True, False])
def test_pack_image_round_trip_and_layout(out_f, in_f, n_mt, n_kg, first):
    rng = np.random.default_rng(out_f * 131 + in_f)
    W = rng.standard_normal((out_f, in_f)).astype(np.float32)
    b = rng.standard_normal(out_f).astype(np.float32)
    img = M.pack_image(W, b, first, n_mt, n_kg)
    assert img.dtype == np.float32 and img.shape == (M.image_floats(n_mt, n_kg),)
    Wp, bp = M.unpack_image(img, first, n_mt, n_kg)
    assert not np.isnan(Wp).any()                                          # every (row, K position) is in exactly one fragment slot
    assert np.array_equal(Wp[:out_f, :in_f], W) and np.array_equal(bp[:out_f], b)
    assert not Wp[out_f:].any() and not Wp[:, in_f:].any() and not bp[out_f:].any()      # padding is zero
    assert np.array_equal(M.pack_image(W, None, first, n_mt, n_kg)[n_mt * n_kg * 256:], np.zeros(16 * n_mt, np.float32))
    # K order: K-step j of group kg, lane group kq
    frag = img[:n_mt * n_kg * 256].reshape(n_mt, n_kg, 4, 16, 4)            # [mt][kg][kq][m][j]
    Wfull = np.zeros((16 * n_mt, 16 * n_kg), np.float32)
    Wfull[:out_f, :in_f] = W
    for t in range(n_kg):
        for kq in range(4):
            for r in range(4):
                # later layers: the B operand lane group kq holds in register r of accumulator tile t is feature 16 t + 4 kq + r;
                # first layer: K-step 4 t + r reads the gathered input rows in natural order, row 16 t + 4 r + kq from lane group kq
                feat = 16 * t + 4 * r + kq if first else 16 * t + 4 * kq + r
                assert np.array_equal(frag[:, t, kq, :, r].reshape(-1), Wfull[:, feat]), (t, kq, r)


def test_pack_image_later_layers_consume_the_accumulator_layout():
    """One layer's accumulators are the next layer's B operands: lane (kq, cl) register (t, r) holds feature 16 t + 4 kq + r, and
    the MFMA K-step (t, r) multiplies component r of fragment (mt, t) of lane (kq, m) with exactly that register."""
    W = np.arange(32 * 32, dtype=np.float32).reshape(32, 32)
    img = M.pack_image(W, None, False, 2, 2)
    for mt in range(2):
        for t in range(2):
            for lane in range(64):
                kq, m = lane // 16, lane % 16
                for r in range(4):
                    assert img[((mt * 2 + t) * 64 + lane) * 4 + r] == W[16 * mt + m, 16 * t + 4 * kq + r]
