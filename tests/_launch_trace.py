"""Launch traces of ``engine.net_tangent`` -- and, further down, of the other passes of a training step through a ResNet coupler -- on
CPU tensors: the launchers are replaced by recorders, so no kernel runs and no GPU is needed.  A trace is the list of (launcher name,
positional arguments, keywords) with every tensor replaced by a name that says WHICH buffer it is (order of first appearance of its
storage), at what offset and in what shape -- two implementations that make the same launches in the same order on the same buffers
give equal traces.  Shared by tests/test_tangent_plan_host.py, tests/test_train_plan_host.py, tests/test_gpu_train_plan.py and
tests/dev/net_tangent_trace.py / train_trace.py (which run the same cases on another checkout of the package)."""
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
        if isinstance(v, E.ActList):
            return ("ActList", tuple(self(x) for x in v), self(v.grouped))
        if isinstance(v, (list, tuple)):
            return tuple(self(x) for x in v)
        if isinstance(v, torch.device):
            return str(v)
        if v is None or isinstance(v, (bool, int, float, str, np.integer)):
            return v if not isinstance(v, np.integer) else int(v)
        raise TypeError(f"launch argument of type {type(v).__name__}")


@contextlib.contextmanager
def recording(E, launchers, names, out):
    """Every launcher of ``launchers`` replaced, by ``setattr`` on the engine module, by a recorder that appends (name, arguments,
    keywords) to ``out`` and returns CPU tensors of the launcher's result shape."""
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
        if name == "primal_regroup":                              # (t, to_grouped): flat, the other layout
            return empty(a[0].numel())
        if name == "relu_bits":                                   # (act (B, C, H, W))
            return E.BitMask(a[0].shape[0], a[0][0, 0].numel(), a[0].shape[1], "cpu")
        if name == "stanh_backward":                              # (dy, dg, y, ...): du like y
            return torch.empty_like(a[2])

    def recorder(name):
        def rec(*a, **k):
            out.append((name, names(a), names(k)))
            return returns(name, a)
        return rec

    saved = {n: getattr(E, n) for n in launchers}
    try:
        for n in launchers:
            setattr(E, n, recorder(n))
        yield
    finally:
        for n, f in saved.items():
            setattr(E, n, f)


def trace(E, net, T, view, acts, save=None, tangent="bf16x3"):
    """-> (launches, (B, N, nc, layout) of the returned stack, its compact flag); ``E`` = the engine module under test."""
    out = []
    with recording(E, LAUNCHERS, _Names(E), out), E.scope(E.KernelConfig(tangent=tangent)):
        yt = E.net_tangent(net, T, view, acts, save=save)
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
def _resnet(cin, nb, cout, hid=HID):
    from cmf_amd import networks
    return networks.get_resnet(cin, [hid] * nb, cout)


def checkerboard_mask(cin, H, W):
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.broadcast_to(((ii + jj) % 2 == 1).astype(np.float32), (cin, H, W)).copy()


@functools.lru_cache(maxsize=None)
def _probe(E, cin, H, W):
    host = E.probe_plan(checkerboard_mask(cin, H, W))
    if host is None:
        return None
    return {"ns": host["ns"], "cls": torch.from_numpy(host["cls"]), "probes": torch.from_numpy(host["probes"]).reshape(-1)}


def net_view(E, H, W, cin, hid, view):
    """The NetView of one of VIEWS on a (cin, H, W) coupler input, all on the CPU."""
    if view == "split":
        return E.NetView(E.Geometry((2 * cin, H, W)), cin)
    live = None
    if view == "checkerboard" and W % 2 == 0:
        live = {"parity": 1, "act_idx": torch.zeros(hid * (H * W // 2), dtype=torch.int32)}
    return E.NetView(E.Geometry((cin, H, W)), cin, mask=torch.from_numpy(checkerboard_mask(cin, H, W)), live=live, probe=_probe(E, cin, H, W))


def resnet_case(E, H, W, cin, cout, nb, nc, B, view, bits, grouped=False):
    """One coupler on CPU tensors -> dict(net, T, view, acts).  ``view``: one of VIEWS; ``bits``: the hidden activations but the last
    are BitMasks (what the primal pass keeps for a batch of whole sample groups), else floats; ``grouped``: sample-grouped floats."""
    net = _resnet(cin, nb, cout)
    hid, HW = E._resnet_parts(net)[0].out_channels, H * W
    nv = net_view(E, H, W, cin, hid, view)
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


# --------------------------------------------------------------------------------------------------
# the other passes of a training step through a ResNet coupler: net_primal, net_cotangent, net_primal_backward
# --------------------------------------------------------------------------------------------------

TRAIN_LAUNCHERS = LAUNCHERS + ("conv_primal", "conv_tangent_wgrad", "conv_tangent_wgrad_batched", "channel_sum", "channel_sum_batched",
                               "primal_regroup", "absmax", "relu_bits", "stanh_backward")
MNIST, HALF, ODD = SHAPES[0], SHAPES[1], SHAPES[3]       # ODD: 7 x 7, the shape the split kernel refuses
TRAIN_NETS = ((MNIST, 64), (HALF, 64), (HALF, 32), (HALF, 128), (ODD, 64))       # hid 32 and 128: the two width fallbacks
TRAIN_NB, TRAIN_B, TRAIN_NC = (0, 1, 2), (8, 16, 32, 48), (16, 32, 64)
CONFIGS = tuple(itertools.product(("bf16x3", "f32"), ("f16x3", "f32", "bf16x3")))          # (tangent, primal)
#: (requested need_acts, training).  The reverse sweep and the primal backward read what a training forward keeps -- True or what
#: ``train_acts_mode`` says -- so False and "bits" (evaluation: the forward sweep alone reads them) are primal passes only.
REQUESTS = ((False, False), ("bits", False), (True, False), (True, True), ("train-if-possible", False), ("train-if-possible", True))


def train_case(shape, hid, nb, B, nc, view, config, need_acts, training):
    kw = dict(zip(("H", "W", "cin", "cout"), shape), hid=hid, nb=nb, B=B, nc=nc, view=view, tangent=config[0], primal=config[1],
              need_acts=need_acts, training=training)
    return " ".join(f"{k}={v}" for k, v in kw.items()), kw


def train_matrix():
    """The full matrix: (label, keywords of ``run_train``).  The primal-only requests do not see ``nc``: they run at the first alone."""
    for (shape, hid), nb, B, view, config, (need, training) in itertools.product(TRAIN_NETS, TRAIN_NB, TRAIN_B, VIEWS, CONFIGS, REQUESTS):
        for nc in TRAIN_NC if need in (True, "train-if-possible") else TRAIN_NC[:1]:
            yield train_case(shape, hid, nb, B, nc, view, config, need, training)


def train_subset():
    """At most 500 rows of ``train_matrix`` that reach every value of every CouplerPlan field: every network, batch size and
    KernelConfig with one block under a checkerboard view, each request once, then the other axes on the 14 x 14 coupler."""
    for (shape, hid), B, config in itertools.product(TRAIN_NETS, TRAIN_B, CONFIGS):
        yield train_case(shape, hid, 1, B, 16, "checkerboard", config, False, False)
        yield train_case(shape, hid, 1, B, 16, "checkerboard", config, "bits", False)
        yield train_case(shape, hid, 1, B, 32, "checkerboard", config, True, False)
        yield train_case(shape, hid, 1, B, 32, "checkerboard", config, "train-if-possible", True)
    for nc, nb, view, need, training in ((16, 1, "checkerboard", "train-if-possible", True), (64, 1, "checkerboard", "train-if-possible", True),
                                         (32, 0, "checkerboard", "train-if-possible", True), (32, 2, "checkerboard", "train-if-possible", True),
                                         (32, 1, "split", "train-if-possible", True), (32, 1, "mask", "train-if-possible", True),
                                         (32, 1, "checkerboard", "train-if-possible", False), (32, 2, "checkerboard", True, True),
                                         (16, 2, "split", True, True)):
        yield train_case(HALF, 64, nb, 32, nc, view, CONFIGS[0], need, training)


def run_train(E, H, W, cin, cout, hid, nb, B, nc, view, tangent, primal, need_acts, training):
    """One row -> {pass: result}: "primal" always; "tangent" (training: the sweep that fills ``saved``), "cotangent" and "backward"
    (training) where the primal pass kept activations for them.  A result is (launches, what the pass returned); the passes share one
    tensor naming, so a buffer one pass hands to the next keeps its name."""
    net = _resnet(cin, nb, cout, hid)
    nv = net_view(E, H, W, cin, E._resnet_parts(net)[0].out_channels, view)
    names, res = _Names(E), {}

    def one(name, fn):
        out = []
        with recording(E, TRAIN_LAUNCHERS, names, out):
            ret = fn()
        res[name] = (out, names(ret))
        return ret

    with E.scope(E.KernelConfig(tangent=tangent, primal=primal)):
        z = torch.zeros(B, *nv.geom.shape)
        need = E.train_acts_mode(net, nv, B, nc=nc) if need_acts == "train-if-possible" else need_acts
        y, g, acts = one("primal", lambda: E.net_primal(net, z, nv, need_acts=need))
        if need_acts in (False, "bits") or acts is None:
            return res
        saved = grads = None
        if training:
            saved, grads = [], {}
            one("tangent", lambda: E.net_tangent(net, E.Tangent(B, nv.geom.N, nc, "panel", "cpu"), nv, acts, save=saved))
        YC, Ct = E.Tangent(B, y[0].numel(), nc, "panel", "cpu"), E.Tangent(B, nv.geom.N, nc, "panel", "cpu")
        one("cotangent", lambda: E.net_cotangent(net, YC, nv, acts, Ct, saved=saved, grads=grads))
        if training:
            one("backward", lambda: E.net_primal_backward(net, z, nv, acts, y, g, torch.zeros_like(y), torch.zeros_like(g), grads,
                                                          torch.zeros_like(z)))
            res["grads"] = ([], names([grads[p] for p in net.parameters() if p in grads]))
    return res


def families(E, launches):
    """The KernelTimer family name of every launch of a trace that carries one (``engine._timed``), in order."""
    out = []
    for name, a, k in launches:
        k = dict(k)
        if name == "conv_tangent":                                # (x_t, x_off, x_np, x_ci, x_px, weight, taps, ..., np_, cin, cout, H, W, nc)
            fo, fmode = k.get("fo"), k.get("fmode", E.F_NONE)
            pbwd = fmode == E.F_NONE and fo is not None and fo[0] != "BitMask" and k.get("fomode") == E.F_SELF_RELU
            out.append(f"conv_tangent_t{a[6]}_ci{a[12]}_co{a[13]}" + ("_primal" if fmode == E.F_SELF_RELU else "_primal_bwd" if pbwd
                                                                        else "_live" if k.get("live") else ""))
        elif name == "conv_tangent_wgrad":                        # (x_t, ..., dw, taps, np_, cin, cout, H, W, nc)
            out.append(f"conv_wgrad_t{a[11]}_ci{a[13]}_co{a[14]}" + ("_primal" if k.get("fmode") == E.F_SELF_RELU else ""))
        elif name == "conv_tangent_wgrad_batched":                # (xs, gys, dws, 6 strides, np_, cin, cout, H, W, nc)
            out.append(f"conv_wgrad_t9_ci{a[10]}_co{a[11]}" + ("_primal" if k.get("fmode") == E.F_SELF_RELU else "") + "_batched")
    return out
