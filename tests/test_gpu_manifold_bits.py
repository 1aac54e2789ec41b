"""The bits of the manifold tools' float64 kernels (csrc/gn_step.hip, curve_step.hip, shoot_step.hip, transport_step.hip,
star_step.hip, weighted_step.hip and what they share, csrc/dense_f64.h): every output array of
``engine.gauss_newton_step``, ``residual_sqnorm``, ``cross_gram``, ``curve_energy``, ``curve_step``, ``metric_solve`` (solve and
apply), ``transport_chain``, ``star_step``, ``star_cross_gram``, ``weighted_gauss_newton_step`` and ``weighted_residual_sqnorm`` on
seeded inputs, bit for bit against the golden files of GOLDEN.  The other tests of these kernels hold them to error bounds; this
one notices a change of a rounded operation, of a summation order or of a failure path that stays inside the bounds.  Needs an
MI355X: run with ``-m gpu``.

Two golden files, each recorded by tests/dev/record_manifold_bits.py, which writes only the file of the families it is given:
  manifold_f64_bits.npz (gn, curve, solve, transport) at commit 88b1635 ("Add ManifoldGeodesic.transport"), before the four kernels
    shared any code;
  manifold_f64_bits_star_weighted.npz (star, weighted) at commit 298d575 ("Add ManifoldProjector.complete"), with that commit's
    library, before the solve tail of gn_step.hip and weighted_step.hip was stated once.
A file is to be re-recorded only by a pull request that changes this arithmetic on purpose and says so.  The files also hold the
SHA-256 of every input: an input that no longer hashes to its record (a changed generator, another numpy) is a failure that asks
for a new recording, never a skip.

The shapes are the smallest that reach every path: d = 1, 17 (two 16-wide thread tiles), 65 (the band's window in the workspace,
LP = 32) and 128 (the widest); D < d; every damping; both layouts; the LU's row swap; the star's padded stack (first = 1); every
weight pattern, and D = 1100, where the weighted kernel's scan of the live rows crosses a 1024-row chunk with a remainder carried
over; and per entry point a refused pivot (code 1) and a non-finite value that is read (code 2)."""
import hashlib
import os

import numpy as np
import pytest

import _curve_step_emulation as CE
import _gn_step_emulation as GN
import _star_step_emulation as SE
import _transport_emulation as TM
import _weighted_step_emulation as WE
import test_gpu_completion as completion
import test_gpu_geodesic as geodesic
import test_gpu_projection as projection
import test_gpu_shoot as shoot
import test_gpu_star as star
import test_gpu_transport as transport
from test_star_host import WEIGHTS

pytestmark = pytest.mark.gpu

NAN = float("nan")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
#: the golden file of each family
GOLDEN = {"gn": "manifold_f64_bits.npz", "curve": "manifold_f64_bits.npz", "solve": "manifold_f64_bits.npz",
          "transport": "manifold_f64_bits.npz", "star": "manifold_f64_bits_star_weighted.npz",
          "weighted": "manifold_f64_bits_star_weighted.npz"}
FAMILIES = list(GOLDEN)

GN_SHAPES = [(3, 5, 1, "panel"), (3, 64, 17, "panel"), (3, 64, 17, "fmajor"), (2, 64, 65, "panel"), (2, 5, 128, "fmajor")]
#: (curves, P, D, d, layout, damping per curve); P = 3 has no cross block, d = 65 and 128 keep the window in the workspace
CURVE_SHAPES = [(2, 3, 5, 1, "panel", [0.0, 10.0]), (2, 4, 64, 17, "panel", [0.0, 1e-3]), (2, 4, 64, 17, "fmajor", [10.0, 0.0]),
                (2, 4, 64, 65, "panel", [1e-3, 10.0]), (1, 9, 5, 128, "fmajor", [1e-3])]
SOLVE_WIDTHS = [1, 17, 65, 128]
TRANSPORT_SHAPES = [(1, 1), (17, 16), (65, 1), (128, 1)]
#: (stars, K, P, D, d, layout, damping per star): every damping of SE.DAMPINGS, and a positive one where D < d; fmajor runs behind
#: the padded stack (first = 1); d = 65 and 128 keep the window in the workspace
STAR_SHAPES = [(2, 1, 3, 5, 1, "panel", [0.0, 1e-3]), (2, 3, 4, 64, 17, "panel", [10.0, 0.0]), (1, 2, 4, 64, 17, "fmajor", [1e-3]),
               (1, 2, 3, 64, 65, "panel", [10.0]), (1, 2, 3, 5, 128, "fmajor", [1e-3])]
#: (B, D, d, layout, the samples of WE.weights that are kept, damping per sample); B = 5: every pattern of WE.PATTERNS; D = 1100:
#: "half" and "third", whose scan crosses a 1024-row chunk and carries a remainder of the live list into the second chunk
WEIGHTED_SHAPES = [(5, 5, 1, "panel", range(5), None), (5, 64, 17, "panel", range(5), None), (5, 64, 17, "fmajor", range(5), None),
                   (1, 64, 65, "panel", [0], [1e-3]), (1, 5, 128, "fmajor", [0], [10.0]), (2, 1100, 17, "panel", [1, 2], [0.0, 1e-3])]
GN_OUT = ("grad", "delta", "stats", "info", "r2", "info_r")              # what the ``run`` of each kernel's own test module returns
CURVE_OUT = ("grad", "delta", "stats", "seg2", "info", "e_seg2", "e_sum", "e_info")
SOLVE_OUT = ("out64", "out32", "stats", "info")


def named(names, arrays):
    return dict(zip(names, arrays))


def gn_cases():
    """(case, inputs, their names, the call that gives {output name: array}) of every Gauss-Newton case"""
    names = ("J", "G", "x", "xhat", "lam")
    for B, D, d, layout in GN_SHAPES:
        lam = np.array([GN.DAMPINGS[b % len(GN.DAMPINGS)] for b in range(B)])
        yield (f"gn/{B}x{D}x{d}/{layout}", GN.inputs(B, D, d) + (lam,), names,
               lambda *a, layout=layout: named(GN_OUT, projection.run(*a, layout)))
    J, G, x, xhat = GN.inputs(7, 64, 5, seed=1)                      # tests/test_gpu_projection.py's failures, and a negative diagonal
    J[1, :, 3] = J[1, :, 1]
    G[1] = GN.gram_by_dots(J[1])
    x[2, 7] = np.inf
    xhat[3, 0] = NAN
    J[4, 3, 4] = NAN
    G[5, 4, 2] = NAN
    G[6, 2, 2] = -1.0
    yield "gn/failures", (J, G, x, xhat, np.zeros(7)), names, lambda *a: named(GN_OUT, projection.run(*a, "panel"))


def curve_cases():
    names = ("J", "G", "C", "xhat", "lam")
    for curves, P, D, d, layout, lam in CURVE_SHAPES:
        J, G, C, xhat = CE.inputs(curves, P, D, d)
        yield (f"curve/{curves}x{P}x{D}x{d}/{layout}", (J, G, C, xhat, np.array(lam)), names,
               lambda *a, P=P, layout=layout: named(CURVE_OUT, geodesic.run(*a, P, layout)))
    for curves, P, D, d, layout in ((2, 4, 64, 17, "panel"), (2, 4, 64, 65, "fmajor"), (1, 4, 5, 128, "panel")):
        J = CE.inputs(curves, P, D, d, seed=4)[0]
        yield (f"curve/cross_gram/{curves}x{P}x{D}x{d}/{layout}", (J,), ("J",),
               lambda J, P=P, d=d, layout=layout: {"cross": geodesic.run_cross(J, P, d, layout)})
    P = 4
    J, G, C, xhat = CE.inputs(3, P, 64, 5, seed=1)
    G[P + 1, 2, 2] = -1.0                                            # curve 1: a negative diagonal at an interior point
    C[2, 0, 2, 4] = NAN                                              # curve 2: a cross block
    yield "curve/failures", (J, G, C, xhat, np.zeros(3)), names, lambda *a: named(CURVE_OUT, geodesic.run(*a, P, "panel"))


def solve_cases():
    names = ("G", "rhs")
    for d in SOLVE_WIDTHS:
        for apply in (False, True):
            G, _, rhs = shoot.inputs(3, d, seed=int(apply))
            yield (f"solve/{d}/{'apply' if apply else 'solve'}", (G, rhs), names,
                   lambda G, rhs, apply=apply: named(SOLVE_OUT, shoot.run(G, rhs, apply)))
    for apply in (False, True):                                      # tests/test_gpu_shoot.py's failures
        G, _, rhs = shoot.inputs(7, 5, seed=2)
        G[1, 2, 2] = -1.0
        G[3, 4, 1] = NAN
        rhs[4, 0] = np.inf
        yield (f"solve/failures/{'apply' if apply else 'solve'}", (G, rhs), names,
               lambda G, rhs, apply=apply: named(SOLVE_OUT, shoot.run(G, rhs, apply)))


def transport_cases():
    names = ("jtj", "cross", "w0")
    for d, m in TRANSPORT_SHAPES:
        yield f"transport/2x3x{d}x{m}", TM.case(2, 3, d, m), names, lambda *a: named(transport.NAMES, transport.run(*a, 3))
    jtj, cross = TM.blocks(TM.pivoting_case()[0])                    # the LU swaps rows
    yield ("transport/pivoting", (jtj, cross, np.arange(15.0).reshape(1, 3, 5) - 7.0), names,
           lambda *a: named(transport.NAMES, transport.run(*a, 2)))
    jtj, cross, w0 = transport.failure_inputs()[1]                   # tests/test_gpu_transport.py's failures, and a negative diagonal
    jtj[0 * 5 + 3, 1, 1] = -1.0
    yield "transport/failures", (jtj, cross, w0), names, lambda *a: named(transport.NAMES, transport.run(*a, 5))


def star_cases():
    names = ("J", "G", "C", "xhat", "w", "lam")
    for stars, K, P, D, d, layout, lam in STAR_SHAPES:
        assert set(SE.DAMPINGS) >= set(lam) and (D >= d or min(lam) > 0.0)
        w = np.tile(WEIGHTS[:K], (stars, 1))
        yield (f"star/{stars}x{K}x{P}x{D}x{d}/{layout}", SE.inputs(stars, K, P, D, d, seed=stars) + (w, np.array(lam)), names,
               lambda *a, P=P, layout=layout: star.run(*a, P, layout))
    for n, D, d, layout in ((4, 64, 17, "panel"), (3, 5, 128, "fmajor")):
        J = CE.inputs(1, n, D, d, seed=8)[0]
        yield f"star/cross_gram/{n}x{D}x{d}/{layout}", (J,), ("J",), lambda J, d=d, layout=layout: {"cross": run_star_cross(J, d, layout)}
    K, P, D, d = 3, 4, 64, 5                                         # tests/test_gpu_star.py's failures, in star 1 of three
    n = K * P
    J, G, C, xhat = SE.inputs(3, K, P, D, d, seed=1)
    w, lam = np.tile(WEIGHTS[:K], (3, 1)), np.zeros(3)

    for what, rows in (("arm_column", [n + P + 2]), ("centre_column", [n + k * P + P - 1 for k in range(K)])):
        Jz = J.copy()                                                # a zero column in one arm, or at every centre copy: code 1
        Jz[rows, :, 3] = 0.0
        J64 = Jz.astype(np.float64)
        Gz, Cz = (J64.transpose(0, 2, 1) @ J64).astype(np.float32), SE.cross_of(Jz).astype(np.float32)
        yield f"star/failures/{what}", (Jz, Gz, Cz, xhat, w, lam), names, lambda *a: star.run(*a, P, "panel")
    Jn, wn = J.copy(), w.copy()
    Jn[n + P + 2, 3, 4] = NAN                                        # a NaN that is read: code 2
    wn[1, 2] = np.inf                                                # a weight that is not finite: code 2
    yield "star/failures/nan", (Jn, G, C, xhat, w, lam), names, lambda *a: star.run(*a, P, "panel")
    yield "star/failures/weight", (J, G, C, xhat, wn, lam), names, lambda *a: star.run(*a, P, "panel")


def run_star_cross(J, d, layout):
    import torch
    from cmf_amd import engine as E
    got = E.star_cross_gram(projection.stack(J, layout), d)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def weighted_cases():
    names = ("J", "w", "x", "xhat", "lam")
    for B, D, d, layout, keep, lam in WEIGHTED_SHAPES:
        J, _, x, xhat = GN.inputs(B, D, d)
        w = WE.weights(max(keep) + 1, D, d)[list(keep)]
        lam = completion.dampings(B) if lam is None else np.array(lam)
        assert len(w) == B == len(lam)
        yield (f"weighted/{B}x{D}x{d}/{layout}", (J, w, x, xhat, lam), names,
               lambda *a, layout=layout: named(completion.NAMES, completion.run(*a, layout)))
    D, d = 64, 5                                                     # tests/test_gpu_completion.py's failures
    J, _, x, xhat = GN.inputs(8, D, d, seed=1)
    w = np.ones((8, D), dtype=np.float32)
    w[:, ::3] = 0.0                                                  # rows 0, 3, 6, ... are dead
    w[:, 1::3] = 2.5
    w[1, 4] = -1.0
    w[2, 5] = NAN
    x[3, 7] = np.inf                                                 # live rows
    xhat[4, 1] = NAN
    J[5, 2, 4] = NAN
    x[6, 3], xhat[6, 6], J[6, 9, 1] = NAN, np.inf, NAN               # dead rows: not an error
    w[7] = 0.0                                                       # no live row: code 1
    yield ("weighted/failures", (J, w, x, xhat, np.zeros(8)), names,
           lambda *a: named(completion.NAMES, completion.run(*a, "panel")))


CASES = {"gn": gn_cases, "curve": curve_cases, "solve": solve_cases, "transport": transport_cases, "star": star_cases,
         "weighted": weighted_cases}


def compute(family):
    """Every case of one family on the GPU: ({'<case>/<output>': array}, {'sha256/<case>/<input>': hex digest})."""
    arrays, hashes = {}, {}
    for case, inputs, in_names, call in CASES[family]():
        for name, a in zip(in_names, inputs):
            hashes[f"sha256/{case}/{name}"] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
        for name, a in call(*inputs).items():
            arrays[f"{case}/{name}"] = np.asarray(a)
    return arrays, hashes


@pytest.mark.parametrize("family", FAMILIES)
def test_outputs_keep_the_recorded_bits(family):
    golden = np.load(os.path.join(GOLDEN_DIR, GOLDEN[family]), allow_pickle=False)
    arrays, hashes = compute(family)
    recorded = [k for k in golden.files if k.split("/")[0] == family or k.split("/")[:2] == ["sha256", family]]
    assert sorted(recorded) == sorted(list(arrays) + list(hashes))   # nothing recorded goes unchecked, nothing new unrecorded
    stale = [k for k, h in hashes.items() if str(golden[k]) != h]
    assert not stale, f"inputs differ from the recording (re-record with tests/dev/record_manifold_bits.py): {stale}"
    moved = []
    for key, got in arrays.items():
        want = golden[key]
        assert got.dtype == want.dtype and got.shape == want.shape, key
        same = np.array_equal(got, want) if got.dtype.kind == "i" else np.array_equal(got, want, equal_nan=True)
        if not same:
            moved.append(f"{key}: {int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())} of {got.size} elements")
    codes = sorted({int(v) for k, a in arrays.items() if k.split("/")[-1] in ("info", "info_r", "e_info") for v in a.reshape(-1)})
    print(f"{family}: {len(arrays)} arrays, {sum(a.nbytes for a in arrays.values())} bytes, info codes {codes}")
    assert codes == [0, 1, 2]                                        # the recording reaches both failure paths
    assert not moved, "\n".join(moved)
