"""Launch traces of ``engine.net_tangent`` on CPU tensors: the launchers are replaced by recorders, so no kernel runs and no GPU is
needed.  A trace is the list of (launcher name, positional arguments, keywords) with every tensor replaced by a name that says WHICH
buffer it is (order of first appearance of its storage), at what offset and in what shape -- two implementations that make the same
launches in the same order on the same buffers give equal traces.  Shared by tests/test_tangent_plan_host.py and
tests/dev/net_tangent_trace.py (which runs the same cases on another checkout of the package)."""
import contextlib
import functools
import hashlib
import itertools

import numpy as np
import torch
import torch.nn as nn

LAUNCHERS = ("conv_tangent", "probe_apply", "seed_panel", "_seed_pack", "_probe_hidden", "gather_primal")
SWITCHES = ("CHECKERBOARD_TAIL", "SKIP_DEAD_ROWS", "FOLD_HEAD", "FOLD_BLOCK", "PROBE_FRONT", "SEED_RESIDUAL")
SHAPES = ((28, 28, 1, 2), (14, 14, 2, 4), (14, 14, 4, 8), (7, 7, 8, 16))          # (H, W, cin, cout)
SIZES = ((16, 2), (32, 16), (64, 32))                                             # (nc, B)
VIEWS = ("checkerboard", "split", "mask")          # live + mask + probe plan | no mask | mask and plan, no live
HID = 64


class _Names:
    """Tensor -> "t<i>+<storage offset>:<shape>"; holds every tensor it has seen, so no address is reused while it lives."""

    def __init__(self, E):
        self.E, self.ids, self.keep = E, {}, []

    def __call__(self, v):
        E = self.E
        if isinstance(v, torch.Tensor):
            self.keep.append(v)
            i = self.ids.setdefault(v.untyped_storage().data_ptr(), len(self.ids))
            return f"t{i}+{v.storage_offset()}:{tuple(v.shape)}"
        if isinstance(v, E.BitMask):
            return ("BitMask", self(v.data), v.np_bytes)
        if isinstance(v, E.Tangent):
            return ("Tangent", self(v.data), v.B, v.N, v.nc, v.layout)
        if isinstance(v, E.NetView):
            return "NetView"
        if isinstance(v, nn.Module):
            return type(v).__name__
        if isinstance(v, dict):
            return tuple((k, self(v[k])) for k in sorted(v))
        if isinstance(v, (list, tuple)):
            return tuple(self(x) for x in v)
        if isinstance(v, torch.device):
            return str(v)
        if v is None or isinstance(v, (bool, int, float, str, np.integer)):
            return v if not isinstance(v, np.integer) else int(v)
        raise TypeError(f"launch argument of type {type(v).__name__}")


def trace(E, net, T, view, acts, save=None, tangent="bf16x3"):
    """-> (launches, (B, N, nc, layout) of the returned stack, its compact flag); ``E`` = the engine module under test."""
    names, out = _Names(E), []
    empty = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype)

    def returns(name, a):
        if name == "seed_panel":                                  # (T, view, H, W)
            col = E.seed_plane(a[2], a[3])
            return dict(panel=empty(a[0].B * a[0].nc * col), np=a[0].nc * col, col=col)
        if name == "_seed_pack":
            return empty(4096, dtype=torch.uint8)
        if name == "_probe_hidden":                               # (conv0, view, plan, H, W, hid, dev)
            return empty(a[3] * a[4] * a[5] * 16 * a[2]["ns"])
        if name == "gather_primal":                               # (src, idx, n_out)
            return empty(a[0].shape[0], a[2])

    def recorder(name):
        def rec(*a, **k):
            out.append((name, names(a), names(k)))
            return returns(name, a)
        return rec

    saved = {n: getattr(E, n) for n in LAUNCHERS}
    try:
        for n in LAUNCHERS:
            setattr(E, n, recorder(n))
        with E.scope(E.KernelConfig(tangent=tangent)):
            yt = E.net_tangent(net, T, view, acts, save=save)
    finally:
        for n, f in saved.items():
            setattr(E, n, f)
    return out, (yt.B, yt.N, yt.nc, yt.layout), bool(getattr(yt, "compact", False))


def digest(result):
    return hashlib.sha1(repr(result).encode()).hexdigest()


@contextlib.contextmanager
def switched_off(E, off):
    """Every switch on but ``off`` (a switch name or None)."""
    saved = {n: getattr(E, n) for n in SWITCHES}
    try:
        for n in SWITCHES:
            setattr(E, n, n != off)
        yield
    finally:
        for n, v in saved.items():
            setattr(E, n, v)


@functools.lru_cache(maxsize=None)
def _resnet(cin, nb, cout):
    from cmf_amd import networks
    return networks.get_resnet(cin, [HID] * nb, cout)


def checkerboard_mask(cin, H, W):
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.broadcast_to(((ii + jj) % 2 == 1).astype(np.float32), (cin, H, W)).copy()


@functools.lru_cache(maxsize=None)
def _probe(E, cin, H, W):
    host = E.probe_plan(checkerboard_mask(cin, H, W))
    if host is None:
        return None
    return {"ns": host["ns"], "cls": torch.from_numpy(host["cls"]), "probes": torch.from_numpy(host["probes"]).reshape(-1)}


def resnet_case(E, H, W, cin, cout, nb, nc, B, view, bits, grouped=False):
    """One coupler on CPU tensors -> dict(net, T, view, acts).  ``view``: one of VIEWS; ``bits``: the hidden activations but the last
    are BitMasks (what the primal pass keeps for a batch of whole sample groups), else floats; ``grouped``: sample-grouped floats."""
    net = _resnet(cin, nb, cout)
    hid, HW = E._resnet_parts(net)[0].out_channels, H * W
    if view == "split":
        nv = E.NetView(E.Geometry((2 * cin, H, W)), cin)
    else:
        live = None
        if view == "checkerboard" and W % 2 == 0:
            live = {"parity": 1, "act_idx": torch.zeros(hid * (HW // 2), dtype=torch.int32)}
        nv = E.NetView(E.Geometry((cin, H, W)), cin, mask=torch.from_numpy(checkerboard_mask(cin, H, W)), live=live, probe=_probe(E, cin, H, W))
    T = E.Tangent(B, nv.geom.N, nc, "panel", "cpu")
    if grouped:
        acts = E.GroupedActs(torch.empty(B // 16, hid, H, W, 16) for _ in range(2 * nb + 1))
    else:
        act = lambda i: E.BitMask(B, HW, hid, "cpu") if bits and 0 < i < 2 * nb else torch.empty(B, hid, H, W)
        acts = [act(i) for i in range(2 * nb + 1)]
    return dict(net=net, T=T, view=nv, acts=acts)


def mlp_case(E, B=8, nc=16):
    from cmf_amd import networks
    net = networks.get_mlp(4, [32, 24], 8)
    return dict(net=net, T=E.Tangent(B, 8, nc, "fmajor", "cpu"), view=E.NetView(E.Geometry((8,)), 4, chan_off=1, chan_step=2),
                acts=[torch.empty(B, 32), torch.empty(B, 24)])


def matrix():
    """The full matrix: (label, case keywords, save, tangent, switch that is off or None)."""
    for (H, W, cin, cout), nb, (nc, B), view, bits, save, tangent, off in itertools.product(
            SHAPES, (0, 1, 2, 3), SIZES, VIEWS, (True, False), (None, []), ("bf16x3", "f32"), (None,) + SWITCHES):
        yield (f"{H}x{W} cin={cin} cout={cout} nb={nb} nc={nc} B={B} view={view} bits={int(bits)} save={save} tangent={tangent} off={off}",
               dict(H=H, W=W, cin=cin, cout=cout, nb=nb, nc=nc, B=B, view=view, bits=bits), save, tangent, off)
    for view, save, tangent in itertools.product(VIEWS, (None, []), ("bf16x3", "f32")):
        yield (f"28x28 cin=1 cout=2 nb=2 nc=64 B=32 view={view} grouped save={save} tangent={tangent} off=None",
               dict(H=28, W=28, cin=1, cout=2, nb=2, nc=64, B=32, view=view, bits=False, grouped=True), save, tangent, None)
    for save, tangent in itertools.product((None, []), ("bf16x3", "f32")):
        yield f"mlp fmajor save={save} tangent={tangent} off=None", None, save, tangent, None


def run(E, kw, save, tangent, off):
    """One row of ``matrix`` -> (case, trace result)."""
    case = mlp_case(E) if kw is None else resnet_case(E, **kw)
    with switched_off(E, off):
        return case, trace(E, **case, save=None if save is None else [], tangent=tangent)
