"""Precision guard (``head.precision_guard``), host side: argument checks, the head attribute, the C ABI entry point
and the program's re-run decision.  No GPU needed."""
import math
import os
import re

import numpy as np
import pytest
import torch

import cmf_amd
from cmf_amd import engine as E
from cmf_amd.densities import NonSquareHeadDensity, PrecisionGuard
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head(name):
    g, meta = load_golden(name)
    dens = cmf_amd.get_density(cmf_amd.get_schema(cmf_amd.get_config(meta["dataset"], **meta["overrides"])), g["x"])
    return dens, next(m for m in dens.modules() if isinstance(m, NonSquareHeadDensity))


def test_guard_defaults_and_export():
    g = PrecisionGuard()
    assert cmf_amd.PrecisionGuard is PrecisionGuard and "PrecisionGuard" in cmf_amd.__all__
    assert g.max_condition == PrecisionGuard.DEFAULT_MAX_CONDITION and 1.0 <= g.max_condition < math.inf
    assert (g.fallback.tangent, g.fallback.primal) == ("f32", "f32")
    assert PrecisionGuard(0).max_condition == 0.0 and PrecisionGuard(math.inf).max_condition == math.inf
    assert PrecisionGuard(np.float32(1e3)).max_condition == 1e3
    cfg = E.KernelConfig(tangent="f32")
    assert PrecisionGuard(10, cfg).fallback is cfg
    assert repr(E.KernelConfig()) == "KernelConfig(tangent='bf16x3', primal='f16x3')"      # not a KernelConfig field


@pytest.mark.parametrize("bad", [-1.0, -math.inf, float("nan")])
def test_guard_rejects_bad_thresholds(bad):
    with pytest.raises(ValueError):
        PrecisionGuard(bad)


@pytest.mark.parametrize("bad", ["1e4", None, True, torch.tensor([1.0])])
def test_guard_rejects_non_numbers(bad):
    with pytest.raises(TypeError):
        PrecisionGuard(bad)


def test_guard_rejects_a_fallback_that_is_not_a_kernel_config():
    with pytest.raises(TypeError):
        PrecisionGuard(1e4, fallback=("f32", "f32"))
    with pytest.raises(TypeError):
        PrecisionGuard(1e4, fallback="f32")


def test_head_attribute_defaults_to_none_and_stays_out_of_the_state_dict():
    dens, head = _head("mini_mnist")
    assert head.precision_guard is None
    before = dens.state_dict()
    head.precision_guard = PrecisionGuard()
    after = dens.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not any("guard" in k for k in after)
    assert "precision_guard" not in dict(head.named_parameters()) and "precision_guard" not in dict(head.named_buffers())


def _header_text():
    return open(os.path.join(ROOT, "include", "cmf_amd.h")).read()


def test_entry_point_is_declared_bound_and_exported():
    import ctypes
    from cmf_amd import _lib
    from cmf_amd.build import build
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    assert re.search(r"int\s+cmf_gram_condition\s*\(", text)
    assert "cmf_gram_condition" in _lib.SIGNATURES
    restype, args = _lib.SIGNATURES["cmf_gram_condition"]
    assert len(args) == 10 and args[4] is ctypes.c_float
    lib = ctypes.CDLL(build(verbose=False))
    assert hasattr(lib, "cmf_gram_condition")
    assert os.path.exists(os.path.join(ROOT, "cmf_amd", "csrc", "gram_cond.hip"))


def test_entry_point_rejects_bad_widths_before_any_launch():
    """CMF_EINVAL for d outside 1 .. 512, a missing workspace above 128 and a NaN threshold: the checks come before the stream
    is touched, so they run without a device (fake non-NULL pointers are never dereferenced)."""
    from cmf_amd import _lib
    lib = _lib.load()
    p = 4096
    call = lambda d, thr=1e4, ws=p: lib.cmf_gram_condition(p, p, d, 4, thr, p, p, p, ws, None)
    assert call(0) == -1 and call(513) == -1 and call(-3) == -1
    assert call(129, ws=None) == -1 and call(512, ws=None) == -1
    assert call(64, thr=float("nan")) == -1
    assert lib.cmf_gram_condition(None, p, 64, 4, 1e4, p, p, p, None, None) == -1


@pytest.mark.parametrize("name,depends", [("c1_sphere", False), ("c2b_hepmass", False), ("mini_mnist", True),
                                          ("c3_mnist_full", True), ("mini_cifar", True)])
def test_rerun_decision_follows_the_coupler_networks(name, depends):
    """Only ResNet couplers run the 3x3 convolutions whose arithmetic KernelConfig picks; an MLP-coupler flow computes the same
    numbers under every configuration, so the guard records its estimate and re-runs nothing."""
    _, head = _head(name)
    assert head.program.depends_on_kernel_config() is depends
