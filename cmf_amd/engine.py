"""Host-side driver of the HIP kernels: tensors in, kernel launches out.

PyTorch provides device memory (caching allocator) and the current HIP stream; every number is
produced by libcmf_amd.so through the C ABI in include/cmf_amd.h.  There is no CPU path: tensors
that are not on a GPU raise.

Layouts
  primal   (B, N) row-major fp32                       -- identical to the reference's tensors
  tangent  ``Tangent``: T(b, r, col), col = Jacobian column, NC = ceil16(#columns)
             'panel'  (B, N, NC)   image nets: one J panel per sample
             'fmajor' (N, B, NC)   MLP nets: feature-major so that a Linear layer is a 1x1
                                   convolution whose "pixels" are the batch samples
"""
import ctypes as C
import math
import threading
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import (F_NONE, F_RELU, F_TANH, F_RAW, F_SELF_RELU, F_RELU_BITS, O_NONE, O_TANH, O_STANH, ConvPrimalArgs,
                   ConvTangentArgs)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def require_gpu(t, what="input"):
    if not t.is_cuda:
        raise RuntimeError(f"cmf_amd: {what} is on {t.device}; the log-density path runs only through the HIP "
                           "kernels on an AMD GPU (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"cmf_amd: {what} must be float32, got {t.dtype}")


def ceil16(n):
    return (int(n) + 15) // 16 * 16


class KernelTimer:
    """Optional live timing of one kernel family with HIP events on the launch stream (bench.py's
    roofline leg).  ``with_events`` brackets a launch with two events; ``summary()`` synchronises once."""

    def __init__(self, select):
        self.select, self.records = select, []

    def wrap(self, name, flops, nbytes, launch):
        if not self.select(name):
            return launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        self.records.append((name, flops, nbytes, e0, e1))

    def reset(self):
        self.records = []

    def by_name(self):
        """{name: (launches, total_ms, flops, bytes)} over the recorded launches."""
        torch.cuda.synchronize()
        out = {}
        for name, fl, by, e0, e1 in self.records:
            n, ms, f, b = out.get(name, (0, 0.0, 0.0, 0.0))
            out[name] = (n + 1, ms + e0.elapsed_time(e1), f + fl, b + by)
        return out

    def summary(self):
        torch.cuda.synchronize()
        n = len(self.records)
        ms = sum(r[3].elapsed_time(r[4]) for r in self.records)
        return {"launches": n, "total_ms": ms, "flops": sum(r[1] for r in self.records),
                "bytes": sum(r[2] for r in self.records)}


class KernelConfig:
    """Which arithmetic the convolution kernels of a head run in (an attribute of ``NonSquareHeadDensity``: ``head.kernels``;
    every ``FlowProgram`` method runs inside ``scope(head.kernels)``, so two heads -- or two threads -- may differ).

    tangent  3x3 hidden TANGENT convolutions (all d Jacobian columns), their transposes and weight gradients:
             "bf16x3" = split-precision bf16 MFMA (hi*hi + hi*lo + lo*hi, fp32 accumulate; fp32-grade on the tangents: errors
             average over K = 576), "f32" = exact fp32 MFMA.  Layers the split kernel does not cover (1x1, cin % 32 != 0, widths
             other than multiples of 14 / 8) always use the fp32 kernel.
    primal   hidden 3x3 PRIMAL convolutions of a ResNet coupler (16 samples in the column slots of the tangent kernels).  The
             relu masks of the Jacobian are taken from these activations, and a pre-activation that lands on the other side of
             zero than in the reference flips a mask, so this arithmetic has to be fp32-grade PER PRODUCT:
             "f16x3" (default) = fp16 split, 11 + 11 significant bits with exact power-of-two operand scales (~2^-22 per product:
             as few mask flips as exact fp32 products, profiles/r04_primal_precision_study.txt) at the bf16 MFMA rate;
             "f32" = exact fp32 MFMA (2.8x slower); "bf16x3" = bf16 split (~2^-16: ~15x more mask flips, median per-sample
             log-det / g_ij error 3e-6 / 1.4e-5 instead of 1e-6 / 2e-7 -- kept as an experiment, never the default)."""
    __slots__ = ("tangent", "primal")

    def __init__(self, tangent="bf16x3", primal="f16x3"):
        assert tangent in ("bf16x3", "f32") and primal in ("f16x3", "f32", "bf16x3")
        self.tangent, self.primal = tangent, primal

    def __repr__(self):
        return f"KernelConfig(tangent={self.tangent!r}, primal={self.primal!r})"


_DEFAULT_CONFIG = KernelConfig()
_tls = threading.local()


def cfg():
    """The calling thread's current KernelConfig (the innermost ``scope``), or the defaults."""
    stack = getattr(_tls, "cfg", None)
    return stack[-1] if stack else _DEFAULT_CONFIG


class scope:
    """``with scope(config):`` -- kernels launched by THIS thread inside the block use ``config`` (re-entrant, nestable)."""

    def __init__(self, config=None, **kw):
        cur = cfg()
        self.config = config if config is not None else KernelConfig(
            **{**{"tangent": cur.tangent, "primal": cur.primal}, **kw})

    def __enter__(self):
        if not hasattr(_tls, "cfg"):
            _tls.cfg = []
        _tls.cfg.append(self.config)
        return self.config

    def __exit__(self, *exc):
        _tls.cfg.pop()
        return False


def _timer():
    return getattr(_tls, "timer", None)


class _use_timer:
    """Install an existing KernelTimer (or None) on the calling thread: autograd runs ``backward`` on its own thread, and the
    timer that was active when the elbo was computed should see the backward kernels too (tools/bench_train.py)."""

    def __init__(self, timer):
        self.timer = timer

    def __enter__(self):
        self.prev = _timer()
        _tls.timer = self.timer
        return self.timer

    def __exit__(self, *exc):
        _tls.timer = self.prev
        return False


class timing:
    """``with timing(select) as t:`` -- launches of THIS thread whose family name ``select`` accepts are bracketed by HIP
    events on the launch stream; ``t.by_name()`` / ``t.summary()`` synchronise once (bench.py's roofline / stages legs)."""

    def __init__(self, select):
        self.timer = KernelTimer(select)

    def __enter__(self):
        self.prev = _timer()
        _tls.timer = self.timer
        return self.timer

    def __exit__(self, *exc):
        _tls.timer = self.prev
        return False


def _timed(name, cost, launch):
    """Run ``launch`` under the calling thread's timer, if it has one, as an entry of the family ``name``; ``cost()`` gives the
    launch's (flops, bytes) and is evaluated only then (it may read arguments the untimed path never touches).  ``name`` None: a
    launch that carries no timer entry."""
    timer = _timer()
    if timer is None or name is None:
        return launch()
    return timer.wrap(name, *cost(), launch)


def _use_bf16x3(taps, cin, W, transpose, H=None, cout=64):
    return cfg().tangent == "bf16x3" and _shape_ok_bf16x3(taps, cin, W, transpose, H, cout)


def _shape_ok_bf16x3(taps, cin, W, transpose, H=None, cout=64):
    """Shapes the split-precision kernel is built for: whole 2 x 14 (or 2 x 8) pixel tiles, whole 64- (or one 32-) channel groups --
    the same for a conv and its transpose (``transpose`` is not read: the tests call this with it, by position)."""
    return (taps == 9 and cin % 32 == 0 and ((W % 14 == 0 and (H is None or H % 2 == 0)) or (W % 8 == 0 and (H is None or H % 4 == 0)))
            and (cout % 64 == 0 or cout == 32))


class Tangent:
    """A stack of Jacobian columns attached to a primal tensor of N elements per sample."""

    def __init__(self, B, N, nc, layout, device, data=None, compact=False):
        self.B, self.N, self.nc, self.layout = int(B), int(N), int(nc), layout
        self.compact = compact            # a checkerboard coupler network's output at its live pixels only (TangentPlan.compact)
        numel = self.B * self.N * self.nc
        self.data = data if data is not None else torch.empty(numel, dtype=torch.float32, device=device)
        assert self.data.numel() >= numel

    @property
    def t_b(self):
        return self.N * self.nc if self.layout == "panel" else self.nc

    @property
    def t_r(self):
        return self.nc if self.layout == "panel" else self.B * self.nc

    def like(self, N):
        return Tangent(self.B, N, self.nc, self.layout, self.data.device)

    @staticmethod
    def from_dense(dense, nc, layout):
        """(B, N, S) torch tensor -> tangent / cotangent stack with S <= nc columns (the rest zero)."""
        B, N, S = dense.shape
        t = Tangent(B, N, nc, layout, dense.device)
        buf = t.data[: B * N * nc].zero_()
        if layout == "panel":
            buf.view(B, N, nc)[:, :, :S] = dense
        else:
            buf.view(N, B, nc)[:, :, :S] = dense.permute(1, 0, 2)
        return t

    def to_dense(self, ncols):
        """(B, N, ncols) torch view/copy for tests and the public jvp API."""
        if self.layout == "panel":
            return self.data[: self.B * self.N * self.nc].view(self.B, self.N, self.nc)[:, :, :ncols]
        return self.data[: self.B * self.N * self.nc].view(self.N, self.B, self.nc).permute(1, 0, 2)[:, :, :ncols]


# --------------------------------------------------------------------------------------------------
# packed weights, cached per parameter version
# --------------------------------------------------------------------------------------------------


class _PackCache:
    """Packed (kernel-layout) copies of weights, rebuilt when the parameter is updated in place
    (``_version``), re-allocated or moved.  Entries hold a weak reference to the parameter and are
    validated by identity: ``id()`` values and device addresses are recycled after garbage collection."""

    def __init__(self):
        self._store = {}
        self.generation = 0
        self._tables = {}                                          # device -> (signature, descriptor table) of the batched refresh
        self._lock = threading.RLock()                             # two threads on one device may share the cache
        self._refreshed = {}                                       # device -> generation its batched refresh last ran for

    def invalidate(self):
        """Every cached pack is stale from now on.  Called by writers that change parameter VALUES without touching the
        tensors' version counters: ``FlatOptimizer.step`` updates the flat buffer with a raw HIP kernel, and a parameter
        whose ``.data`` is a view of that buffer keeps ``_version`` 0 whatever happens to the storage."""
        self.generation += 1

    def get(self, weight, taps, transpose=False, bf16x3=False):
        """``bf16x3``: False = cmf_pack_weight's floats, True / "bf16x3" = the split-precision pack, "f16x3" = the fp16 pack
        (scaled by a power of two, 16-byte trailer).  Thread-safe: the whole lookup / rebuild runs under the cache's lock, and a
        pack built by a launch on ANOTHER stream is ordered before the caller's stream through the event recorded behind that
        launch (two threads on one device with a stream each)."""
        with self._lock:
            out, order = self._get(weight, taps, transpose, bf16x3)
            self._wait(order)
            return out

    @staticmethod
    def _mark():
        """(stream id, event recorded on it now): what a later consumer on a different stream has to wait for."""
        if torch.cuda.is_current_stream_capturing():
            return None
        st = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(st)
        return [st.cuda_stream, ev]

    @staticmethod
    def _wait(order):
        if order is None or order[1] is None:                        # (no launch to order against, or known complete)
            return
        if torch.cuda.is_current_stream_capturing():                  # (capture follows warm-up calls on the capture stream's side)
            return
        if order[1].query():
            order[1] = None                                           # complete for every stream from now on: no more host calls
            return
        st = torch.cuda.current_stream()
        if st.cuda_stream != order[0]:
            st.wait_event(order[1])

    def _get(self, weight, taps, transpose, bf16x3):
        import weakref
        bf16x3 = {False: 0, True: 1, "bf16x3": 1, "f16x3": 2, 0: 0, 1: 1, 2: 2}[bf16x3]      # = cmf_pack_desc.kind
        key = (id(weight), bool(transpose), bf16x3)
        ver = (weight._version, weight.data_ptr(), weight.device, tuple(weight.shape), self.generation)
        hit = self._store.get(key)
        if hit is not None and hit[0]() is weight and hit[1] == ver:
            return hit[2], hit[4]
        if (hit is not None and hit[0]() is weight and hit[1][:4] == ver[:4] and self.BATCHED_REFRESH
                and self._refreshed.get(weight.device) != self.generation and not torch.cuda.is_current_stream_capturing()):
            # only the generation moved: an optimiser step rewrote the parameter VALUES (FlatOptimizer.step -> invalidate()).
            # Every pack of the model is stale in the same way: rebuild them all in ONE launch instead of one launch each --
            # once per generation and device (entries it had to skip are rebuilt singly below), never inside a graph capture
            # (the descriptor table is a host -> device copy)
            self._refresh_generation(weight.device)
            self._refreshed[weight.device] = self.generation
            hit = self._store.get(key)
            if hit[1] == ver:
                return hit[2], hit[4]
        lib = _lib.load()
        cout, cin = int(weight.shape[0]), int(weight.shape[1])
        n = C.c_longlong(0)
        w = weight.detach().contiguous()
        # a stale entry's buffer is reused when the size still fits (training: every pack is rebuilt after every optimiser step)
        old = hit[2] if hit is not None and hit[0]() is weight and hit[2].device == weight.device else None
        buf = lambda nbytes, dt: old if old is not None and old.dtype == dt and old.numel() * old.element_size() == nbytes \
            else torch.empty(nbytes // torch.empty(0, dtype=dt).element_size(), dtype=dt, device=weight.device)
        if bf16x3:
            if transpose:                                  # the adjoint operator: channels swapped, taps flipped -- by the pack kernel
                cout, cin = cin, cout
            fn, what = ((lib.cmf_pack_weight_bf16x3_t, "cmf_pack_weight_bf16x3_t") if bf16x3 == 1 else
                        (lib.cmf_pack_weight_f16x3, "cmf_pack_weight_f16x3"))
            _lib.check(fn(None, None, cout, cin, int(transpose), C.byref(n), None), "pack size")
            out = buf(n.value, torch.uint8)
            _lib.check(fn(_p(w), _p(out), cout, cin, int(transpose), None, _stream()), what)
        else:
            _lib.check(lib.cmf_pack_weight(None, None, cout, cin, taps, int(transpose), C.byref(n), None), "pack size")
            out = buf(4 * n.value, torch.float32)
            _lib.check(lib.cmf_pack_weight(_p(w), _p(out), cout, cin, taps, int(transpose), None, _stream()), "cmf_pack_weight")
        if len(self._store) > 4096:                                   # drop entries whose parameter is gone
            self._store = {k: v for k, v in self._store.items() if v[0]() is not None}
        order = self._mark()
        self._store[key] = (weakref.ref(weight), ver, out, int(taps), order)
        return out, order

    #: False: every stale pack is rebuilt by its own launch on first use (rounds 1 - 2)
    BATCHED_REFRESH = True

    def _refresh_generation(self, device):
        """Re-pack, in one ``cmf_pack_weights_batched`` launch, every entry on ``device`` whose parameter is alive and unchanged
        but for the generation counter (its values were rewritten under it by the fused optimiser step)."""
        todo = []
        for key, (ref, ver, out, taps, _) in list(self._store.items()):
            w = ref()
            if (w is None or ver[4] == self.generation or w.device != device or not w.is_contiguous()
                    or (w._version, w.data_ptr(), w.device, tuple(w.shape)) != ver[:4]):
                continue
            if not isinstance(w, nn.Parameter):
                # a DERIVED tensor (masked MADE weight, L U product: engine.DERIVED): its values are still the old ones until its
                # own rebuild copies the new ones in (bumping _version); re-packing it now would stamp a stale pack as fresh
                continue
            todo.append((key, w, ver, out, taps))
        if not todo:
            return
        desc = np.dtype([("w", "<u8"), ("out", "<u8"), ("total", "<i8"), ("cout", "<i4"), ("cin", "<i4"), ("taps", "<i4"),
                         ("transpose", "<i4"), ("kind", "<i4"), ("reserved", "<i4")])            # = cmf_pack_desc (include/cmf_amd.h)
        sig = tuple((key, w.data_ptr(), out.data_ptr()) for key, w, ver, out, taps in todo)
        cached = self._tables.get(device)
        if cached is not None and cached[0] == sig:
            table = cached[1]
        else:
            arr = np.zeros(len(todo), dtype=desc)
            for i, (key, w, ver, out, taps) in enumerate(todo):
                _, transpose, bf16x3 = key
                cout, cin = int(w.shape[0]), int(w.shape[1])
                if bf16x3 and transpose:
                    cout, cin = cin, cout
                total = out.numel() * out.element_size()
                total = (total - 16) // 2 if bf16x3 == 2 else total // (2 if bf16x3 else 4)     # kind 2: 16-byte trailer
                arr[i] = (w.data_ptr(), out.data_ptr(), total, cout, cin, taps, int(transpose), int(bf16x3), 0)
            table = torch.from_numpy(arr.view(np.uint8).copy()).to(device)
            self._tables[device] = (sig, table)
        _lib.check(_lib.load().cmf_pack_weights_batched(_p(table), len(todo), _stream()), "cmf_pack_weights_batched")
        order = self._mark()                                          # one event behind the one launch, shared by its entries
        for key, w, ver, out, taps in todo:
            self._store[key] = (self._store[key][0], ver[:4] + (self.generation,), out, taps, order)


PACKS = _PackCache()


# --------------------------------------------------------------------------------------------------
# thin wrappers over the C ABI
# --------------------------------------------------------------------------------------------------


def conv_primal(x_ptr_t, x_off, x_b, x_c, x_px, weight, taps, bias, y, y_b, y_c, y_px, B, cin, cout, H, W,
                imode=F_NONE, mask=None, f_c=0, f_px=0, omode=O_NONE, sw=None, sb=None, g=None, res=None):
    """One primal conv/linear launch.  ``x_ptr_t`` is the tensor holding the input, ``x_off`` an element offset."""
    lib = _lib.load()
    a = ConvPrimalArgs()
    a.x = C.c_void_p(x_ptr_t.data_ptr() + 4 * int(x_off)); a.x_b, a.x_c, a.x_px = int(x_b), int(x_c), int(x_px)
    a.f = _p(mask); a.f_c, a.f_px = int(f_c), int(f_px); a.imode = imode
    a.w = _p(PACKS.get(weight, taps)); a.bias = _p(bias); a.sw = _p(sw); a.sb = _p(sb)
    a.y = _p(y); a.y_b, a.y_c, a.y_px = int(y_b), int(y_c), int(y_px)
    a.g = _p(g)
    a.r = _p(res); a.r_b, a.r_c, a.r_px = int(y_b), int(y_c), int(y_px)
    a.omode = omode
    a.B, a.cin, a.cout, a.H, a.W, a.taps = int(B), int(cin), int(cout), int(H), int(W), int(taps)
    _lib.check(lib.cmf_conv_primal(C.byref(a), _stream()), "cmf_conv_primal")


def conv_tangent(x_t, x_off, x_np, x_ci, x_px, weight, taps, y_t, y_np, y_co, y_px, np_, cin, cout, H, W, nc,
                 fmode=F_NONE, f=None, f_np=0, f_ci=0, f_px=0, res_t=None, transpose=False, bias=None, f_group=1,
                 x_sl=16, y_sl=16, precision=None, y_off=0, res_off=0, fo=None, fo_np=0, fo_co=0, fo_px=0, fomode=F_NONE,
                 mask_out=None, mask_np=0, amax_in=None, amax_out=None, item_channels=0, live=0, res_np=None, ymask=None, head=None,
                 seed=None):
    """``fo`` = OUTPUT-side factor (reverse sweep, fp32 kernel only); ``y_off`` / ``res_off`` = element offsets into
    ``y_t`` / ``res_t`` (in-place accumulation into a strided view of a larger tensor).  ``precision`` "f16x3": the fp16 split
    kernel of the primal pass (``amax_in`` / ``amax_out``: one-float device tensors, the input-range chain).  ``live`` 1 / 2:
    checkerboard output (split-precision kernel only): the pixels with (row + col) % 2 == live - 1, stored compactly
    (``res_np``: sample stride of the residual, a FULL image then; the other residual strides are y's).  ``ymask`` (a BitMask over
    the output channels, split-precision kernel only): store filter -- output rows whose bit is clear are not written.
    ``head`` = dict(weight=<the 1x1 conv's weight (cout', 64, 1, 1)>, act=<float activation (np, 64, H, W) it takes relu' from>):
    FOLDED HEAD (csrc/conv_head.hip) -- this launch is a coupler network's last hidden conv AND the 1x1 conv behind it; ``y_t`` and
    its strides then describe the 1x1 conv's output (np, cout', pixels, nc) (compact pixels under ``live``), ``res_t`` the block's
    input h (slice-major like x, required), ``weight`` goes in raw, and the factor must be a BitMask's.  With a further entry
    ``conv1=dict(weight=<the block's conv1 weight>, mask=<BitMask between conv1 and conv2>)``: FOLDED BLOCK
    (csrc/conv_block_head.hip) -- the launch is the block's conv1 as well; ``x_t`` is then the block's input h (its own residual, no
    ``res_t``) and the factor the BitMask of the activation in front of conv1.
    ``seed`` = dict(panel=, np=, col=, pack=) (``seed_panel`` / ``_seed_pack``): SEEDED RESIDUAL -- the launch is block 0's conv2 and
    forms its residual conv0(mask . v) itself from the one-channel seed panel; no ``res_t``, the factor must be a BitMask's."""
    lib = _lib.load()
    a = ConvTangentArgs()
    if head is not None:
        assert (precision or cfg().tangent) == "bf16x3" and not transpose and bias is None and fo is None and ymask is None \
            and mask_out is None, "the folded head replaces the split-precision forward conv + 1x1 conv only"
        return _conv_tangent_head(lib, a, x_t, x_off, x_np, x_ci, x_px, weight, taps, y_t, y_np, y_co, y_px, np_, cin, cout, H, W, nc,
                                  fmode, f, f_np, res_t, res_off, res_np, x_sl, y_off, live, head)
    a.x = C.c_void_p(x_t.data_ptr() + 4 * int(x_off)); a.x_np, a.x_ci, a.x_px = int(x_np), int(x_ci), int(x_px)
    a.f = _p(f); a.f_np, a.f_ci, a.f_px = int(f_np), int(f_ci), int(f_px); a.fmode = fmode
    # split-precision kernel: any input factor without output factor, or NO input factor with an optional relu' BIT MASK on the
    # output (no residual then): the transposed convs of the reverse sweep
    obits = isinstance(fo, BitMask)
    # ... or with the residual IN PLACE (res_t is y_t at the same offset: y <- y + mask . conv(x), the reverse sweep's skip connection)
    inplace = res_t is not None and res_t.data_ptr() == y_t.data_ptr() and int(res_off) == int(y_off)
    precision = precision or cfg().tangent
    split = (precision == "bf16x3" and _shape_ok_bf16x3(taps, cin, W, transpose, H, cout)
             and not (bias is not None and cout > 64)
             and ((fmode != F_NONE and fo is None) or
                  (fmode == F_NONE and (fo is None or (obits and (res_t is None or inplace) and cout % 64 == 0)))))
    # fp16 split kernel: the primal pass's forward form (the input's own relu) or its backward form (plain cotangent in, per-column
    # relu' of a float activation laid out like y on the way out, optional residual: net_primal_backward)
    pbwd = fmode == F_NONE and fo is not None and not obits and fomode == F_SELF_RELU
    # (the split kernels fetch their per-channel constants once per launch: a bias only with a single 64-channel group)
    f16 = (precision == "f16x3" and cout % 64 == 0 and _shape_ok_bf16x3(taps, cin, W, transpose, H, cout)
           and not (bias is not None and cout > 64)
           and ((fmode == F_SELF_RELU and fo is None and not transpose) or (pbwd and bias is None and mask_out is None)))
    assert not obits or split, "bit-mask output factors are applied by the split-precision kernel only"
    if obits:
        fo, fo_np, fo_co, fo_px, fomode = fo.data, fo.np_bytes, 0, 0, F_RELU_BITS
    a.w = _p(PACKS.get(weight, taps, transpose, bf16x3="f16x3" if f16 else split))
    a.y = C.c_void_p(y_t.data_ptr() + 4 * int(y_off)); a.y_np, a.y_co, a.y_px = int(y_np), int(y_co), int(y_px)
    a.r = None if res_t is None else C.c_void_p(res_t.data_ptr() + 4 * int(res_off))
    a.r_np, a.r_co, a.r_px = int(y_np if res_np is None else res_np), int(y_co), int(y_px)
    a.fo = _p(fo); a.fo_np, a.fo_co, a.fo_px, a.fomode = int(fo_np), int(fo_co), int(fo_px), int(fomode)
    a.mask_out = _p(mask_out); a.mask_np = int(mask_np)
    assert not (fmode == F_RELU_BITS and not split), "bit-mask factors are read by the split-precision kernel only"
    assert not (mask_out is not None and split), "sign bits are written by the fp32 and the fp16-split kernels only"
    a.amax_in, a.amax_out = (_p(amax_in), _p(amax_out)) if f16 else (None, None)
    a.live = int(live)
    assert not live or split, "checkerboard output is the split-precision kernel's"
    assert ymask is None or split, "the store filter is the split-precision kernel's"
    if ymask is not None:
        a.ymask, a.ymask_np = _p(ymask.data), int(ymask.np_bytes)
    if seed is not None:
        assert split and res_t is None and fmode == F_RELU_BITS, "the seeded residual is the split-precision kernel's, bit-mask factor"
        a.seed, a.seed_np, a.seed_col, a.seed_w = _p(seed["panel"]), int(seed["np"]), int(seed["col"]), _p(seed["pack"])
    a.np, a.cin, a.cout, a.H, a.W, a.nc, a.taps = int(np_), int(cin), int(cout), int(H), int(W), int(nc), int(taps)
    a.bias = _p(bias); a.f_group = int(f_group)
    a.x_sl, a.y_sl, a.r_sl = int(x_sl), int(y_sl), int(y_sl)
    fn, what = ((lib.cmf_conv_tangent_f16x3, "cmf_conv_tangent_f16x3") if f16 else
                (lib.cmf_conv_tangent_bf16x3, "cmf_conv_tangent_bf16x3") if split else (lib.cmf_conv_tangent, "cmf_conv_tangent"))
    launch = lambda: _lib.check(fn(C.byref(a), _stream()), what)
    if f16 and item_channels:                               # tests / probes: the item size cmf_conv_tangent_f16x3 would pick itself
        launch = lambda: _lib.check(lib.cmf_conv_tangent_f16x3_item(C.byref(a), int(item_channels), _stream()), "cmf_conv_tangent_f16x3_item")
    if fmode == F_SELF_RELU and not f16 and _lib.tracing():
        run = launch

        def launch():                                       # traced: a primal launch of a tangent kernel (bench.py's stages)
            with _lib.role("primal"):
                run()

    def cost():
        # algorithmic work of this launch: 2*cin*cout*taps FLOP per output pixel and Jacobian column; every input,
        # output and residual element crosses HBM once (4 bytes each)
        px_in = float(H) * W * nc * np_
        px = px_in * (0.5 if live else 1.0)                 # checkerboard output: half the output pixels (and residual reads), every input pixel
        # seeded residual: + the seed K-step's 9 taps of one channel, + the panel's bytes instead of a residual's
        return (2.0 * (cin + (1 if seed is not None else 0)) * cout * taps * px,
                4.0 * (px_in * cin + px * (cout + (cout if res_t is not None else 0))
                       + (float(seed["np"]) * np_ if seed is not None else 0.0)))
    return _timed(f"conv_tangent_t{taps}_ci{cin}_co{cout}" + ("_primal" if fmode == F_SELF_RELU else "_primal_bwd" if pbwd else "_live" if live else ""),
                  cost, launch)


def _conv_tangent_head(lib, a, x_t, x_off, x_np, x_ci, x_px, weight, taps, y_t, y_np, y_co, y_px, np_, cin, cout, H, W, nc, fmode, f,
                       f_np, res_t, res_off, res_np, x_sl, y_off, live, head):
    """``conv_tangent(..., head=)``: fill the head fields and launch; the C entry validates the shapes (CMF_EINVAL otherwise)."""
    wf, act = head["weight"], head["act"]
    hc = int(wf.shape[0])
    w2, wf = weight.detach(), wf.detach().reshape(hc, -1)
    assert w2.is_contiguous() and wf.is_contiguous() and act.is_contiguous() and w2.dtype == wf.dtype == act.dtype == torch.float32
    a.x = C.c_void_p(x_t.data_ptr() + 4 * int(x_off)); a.x_np, a.x_ci, a.x_px, a.x_sl = int(x_np), int(x_ci), int(x_px), int(x_sl)
    a.f = _p(f); a.f_np = int(f_np); a.fmode = int(fmode)
    a.w = _p(w2)
    a.r = None if res_t is None else C.c_void_p(res_t.data_ptr() + 4 * int(res_off))
    a.r_np, a.r_co, a.r_px, a.r_sl = int(x_np if res_np is None else res_np), int(x_ci), int(x_px), int(x_sl)
    a.np, a.cin, a.cout, a.H, a.W, a.nc, a.taps, a.live = int(np_), int(cin), int(cout), int(H), int(W), int(nc), int(taps), int(live)
    blk = head.get("conv1")
    if blk is not None:                                     # folded block: x is h, f its mask; conv1's pack and the mask behind it
        assert res_t is None and isinstance(blk["mask"], BitMask), "the folded block reads h as x and takes relu'(c1) from a BitMask"
        a.block_w1 = _p(_block_pack(blk["weight"], x_t.device))
        a.block_m1, a.block_m1_np = _p(blk["mask"].data), int(blk["mask"].np_bytes)
    a.head_w, a.head_cout = _p(wf), hc
    a.head_a = _p(act); a.head_a_np, a.head_a_c, a.head_a_px = int(cin) * H * W, H * W, 1
    a.head_y = C.c_void_p(y_t.data_ptr() + 4 * int(y_off)); a.head_y_np, a.head_y_co, a.head_y_px = int(y_np), int(y_co), int(y_px)
    launch = lambda: _lib.check(lib.cmf_conv_tangent_bf16x3(C.byref(a), _stream()), "cmf_conv_tangent_bf16x3")

    def cost():
        # what the launch executes: per output pixel hc * 64 * 576 FMAs for E, then hc * 640 per column; u crosses HBM once (counted
        # whole: the live fraction is data), h at the output pixels, the activation and yt
        px_out = float(H) * W * np_ * (0.5 if live else 1.0)
        if blk is not None:
            # folded block: + the coefficient build (9 hc rows x 64 x 576 per output pixel, three bf16 products each), the apply's hc *
            # 1600 FMAs per column; h crosses HBM once, the two bit masks, the activation and yt
            return (2.0 * hc * px_out * (cin * taps * cout + 3 * taps * cin * taps * cout + 25 * cout * nc),
                    4.0 * (float(H) * W * np_ * (nc * cin + 4) + px_out * (cout + nc * hc)))
        return (2.0 * hc * px_out * (cin * taps * cout + (cin * taps + cout) * nc),
                4.0 * (float(H) * W * np_ * nc * cin + px_out * (nc * cout + cout + nc * hc)))
    return _timed(f"conv_tangent_t{taps}_ci{cin}_co{cout}" + ("_live" if live else ""), cost, launch)


_WGRAD_WS = {}


def conv_tangent_wgrad(x_t, x_off, x_np, x_ci, x_px, gy_t, gy_off, y_np, y_co, y_px, dw, taps, np_, cin, cout, H, W, nc,
                       fmode=F_NONE, f=None, f_np=0, f_ci=0, f_px=0, f_group=1, x_sl=16, y_sl=16, precision=None):
    """dw (cout, cin, kh, kw) += weight gradient of the tangent conv described like ``conv_tangent``'s forward launch;
    ``gy_t`` (+ ``gy_off`` elements) is the cotangent of y with y's strides.  fp32 factor tensors only."""
    lib = _lib.load()
    assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == cout * cin * taps
    a = ConvTangentArgs()
    a.x = C.c_void_p(x_t.data_ptr() + 4 * int(x_off)); a.x_np, a.x_ci, a.x_px = int(x_np), int(x_ci), int(x_px)
    fbits = isinstance(f, BitMask)                                   # relu' as a bit mask: the split kernel only
    if fbits:
        f, f_np, f_ci, f_px, fmode = f.data, f.np_bytes, 0, 0, F_RELU_BITS
    a.f = _p(f); a.f_np, a.f_ci, a.f_px = int(f_np), int(f_ci), int(f_px); a.fmode = fmode
    a.y_np, a.y_co, a.y_px = int(y_np), int(y_co), int(y_px)
    a.np, a.cin, a.cout, a.H, a.W, a.nc, a.taps = int(np_), int(cin), int(cout), int(H), int(W), int(nc), int(taps)
    a.f_group = int(f_group)
    a.x_sl, a.y_sl = int(x_sl), int(y_sl)
    need = int(lib.cmf_conv_tangent_wgrad_ws(C.byref(a)))
    key = (x_t.device, torch.cuda.current_stream().cuda_stream)      # one workspace per device and stream (re-entrant)
    ws = _WGRAD_WS.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = _WGRAD_WS[key] = torch.empty(need // 4, dtype=torch.float32, device=x_t.device)
    gy = C.c_void_p(gy_t.data_ptr() + 4 * int(gy_off))
    # split-precision kernel (operands shared through LDS) where the forward convs use one: whole 64-channel blocks, column pairs
    split = ((precision or cfg().tangent) == "bf16x3" and taps == 9 and cin % 64 == 0 and cout % 64 == 0 and nc % 32 == 0
             and fmode in (F_NONE, F_RELU, F_SELF_RELU, F_RELU_BITS) and f_group <= 1)
    assert not fbits or split, "bit-mask factors are read by the split-precision weight-gradient kernel only"
    fn, what = (lib.cmf_conv_tangent_wgrad_bf16x3, "cmf_conv_tangent_wgrad_bf16x3") if split else \
               (lib.cmf_conv_tangent_wgrad, "cmf_conv_tangent_wgrad")
    launch = lambda: _lib.check(fn(C.byref(a), gy, _p(dw), _p(ws), need, _stream()), what)

    def cost():
        px = float(H) * W * nc * np_
        return 2.0 * cin * cout * taps * px, 4.0 * px * (cin + cout)
    return _timed(f"conv_wgrad_t{taps}_ci{cin}_co{cout}" + ("_primal" if fmode == F_SELF_RELU else ""), cost, launch)


def conv_tangent_wgrad_batched(xs, gys, dws, x_np, x_ci, x_px, y_np, y_co, y_px, np_, cin, cout, H, W, nc, fmode=F_NONE, x_sl=16, y_sl=16):
    """``conv_tangent_wgrad`` for up to 16 problems of ONE shape (lists of input tensors, cotangent tensors and weight-gradient
    tensors) in one launch of the split-precision kernel: the 256 persistent workgroups are split over the problems.  For launches
    that are a few dozen image rows each (the primal weight gradients of a coupler at a training shard's sample groups)."""
    lib = _lib.load()
    n = len(xs)
    assert n == len(gys) == len(dws) and 1 <= n <= _lib.WGRAD_MAX_BATCH and fmode in (F_NONE, F_SELF_RELU)
    assert cin % 64 == 0 and cout % 64 == 0 and nc % 32 == 0
    a = ConvTangentArgs()
    a.x = _p(xs[0]); a.x_np, a.x_ci, a.x_px = int(x_np), int(x_ci), int(x_px)
    a.fmode = fmode
    a.y_np, a.y_co, a.y_px = int(y_np), int(y_co), int(y_px)
    a.np, a.cin, a.cout, a.H, a.W, a.nc, a.taps = int(np_), int(cin), int(cout), int(H), int(W), int(nc), 9
    a.f_group = 1
    a.x_sl, a.y_sl = int(x_sl), int(y_sl)
    need = int(lib.cmf_conv_tangent_wgrad_ws(C.byref(a)))
    key = (xs[0].device, torch.cuda.current_stream().cuda_stream)
    ws = _WGRAD_WS.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = _WGRAD_WS[key] = torch.empty(need // 4, dtype=torch.float32, device=xs[0].device)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    for dw in dws:
        assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == cout * cin * 9
    launch = lambda: _lib.check(lib.cmf_conv_tangent_wgrad_bf16x3_batched(C.byref(a), n, arr(xs), arr(gys), arr(dws), _p(ws), need, _stream()),
                                "cmf_conv_tangent_wgrad_bf16x3_batched")

    def cost():
        px = float(H) * W * nc * np_ * n
        return 2.0 * cin * cout * 9 * px, 4.0 * px * (cin + cout)
    return _timed(f"conv_wgrad_t9_ci{cin}_co{cout}" + ("_primal" if fmode == F_SELF_RELU else "") + "_batched", cost, launch)


def primal_regroup(t, to_grouped):
    """(B, N) <-> (B/16, N, 16): sample-grouped layout used to run primal data through the tangent kernels."""
    B = t.shape[0] if to_grouped else t.shape[0] * 16
    N = t[0].numel() if to_grouped else t[0].numel() // 16
    out = torch.empty(t.numel(), dtype=torch.float32, device=t.device)
    _lib.check(_lib.load().cmf_primal_regroup(_p(t), _p(out), B, N, int(to_grouped), _stream()), "cmf_primal_regroup")
    return out


def absmax(t, out):
    """out[0] = max(out[0], max |t|) for a flat fp32 tensor (the input-range word of the fp16-split primal convs)."""
    _lib.check(_lib.load().cmf_absmax(_p(t), t.numel(), _p(out), _stream()), "cmf_absmax")


def gather_primal(src, idx, n_out, out=None):
    """out(b, r) = idx[r] >= 0 ? src(b, idx[r]) : 0.  src: (B, N...) contiguous."""
    B = src.shape[0]
    src2 = src.reshape(B, -1)
    if out is None:
        out = torch.empty(B, n_out, dtype=torch.float32, device=src.device)
    _lib.check(_lib.load().cmf_gather_primal(_p(src2), src2.shape[1], _p(out), n_out, _p(idx), n_out, B, _stream()),
               "cmf_gather_primal")
    return out


def gather_tangent(T, idx, n_out):
    out = T.like(n_out)
    _lib.check(_lib.load().cmf_gather_tangent(_p(T.data), T.t_b, T.t_r, _p(out.data), out.t_b, out.t_r, _p(idx), n_out,
                                              T.nc, T.B, _stream()), "cmf_gather_tangent")
    return out


def expand_columns(T, nc_out, colmap):
    """A panel-layout tangent stack with ``nc_out`` column slots: column c = column ``colmap[c]`` of ``T`` (or zero where -1)."""
    assert T.layout == "panel"
    out = Tangent(T.B, T.N, nc_out, "panel", T.data.device, compact=T.compact)
    _lib.check(_lib.load().cmf_expand_columns(_p(T.data), T.nc, _p(out.data), int(nc_out), _p(colmap), T.B * T.N, _stream()),
               "cmf_expand_columns")
    return out


def seed_tangent(B, N, nc, layout, col_of, d, device, eps=None):
    T = Tangent(B, N, nc, layout, device)
    S = 0 if eps is None else int(eps.shape[2])
    _lib.check(_lib.load().cmf_seed_tangent(_p(T.data), T.t_b, T.t_r, _p(col_of), N, nc, _p(eps), d, S, B, _stream()),
               "cmf_seed_tangent")
    return T


def _y_rows(y, B):
    """(y as (rows, n), sample stride) of a network output: a one-row ``y`` is SHARED by all B samples (stride 0) -- the output of a
    coupler network whose input is structurally zero is the same for every sample (``net_primal_zero_input``)."""
    y2 = y.view(y.shape[0], -1)
    assert y.shape[0] in (1, B)
    return y2, (0 if y.shape[0] == 1 and B > 1 else y2.shape[1])


def _t3(T):
    return (None, 0, 0) if T is None else (_p(T.data), T.t_b, T.t_r)


def acl_primal(z, y, maps, decode, lj=None):
    B = z.shape[0]
    z2 = z.view(B, -1)
    y2, y_b = _y_rows(y, B)
    _lib.check(_lib.load().cmf_acl_primal(_p(z2), z2.shape[1], _p(y2), y_b, _p(maps["zi"]), _p(maps["si"]),
                                          _p(maps["ti"]), maps["n"], B, int(decode), _p(lj), _stream()), "cmf_acl_primal")


def acl_tangent(T, YT, z, y, g, maps):
    """``YT`` None: the network's tangent is identically zero (structurally-zero network input): T_mod <- e^{-s} T_mod."""
    B = z.shape[0]
    z2 = z.view(B, -1)
    y2, y_b = _y_rows(y, B)
    launch = lambda: _lib.check(_lib.load().cmf_acl_tangent(_p(T.data), T.t_b, T.t_r, *_t3(YT), T.nc, _p(z2),
                                                            z2.shape[1], _p(y2), y_b, _p(g), _p(maps["zi"]), _p(maps["si"]),
                                                            _p(maps["ti"]), maps["n"], B, _stream()), "cmf_acl_tangent")

    def cost():
        # coupling pass, per modified element: tangent rows v, s-dot, t-dot in (3 x NC floats), one row out, 5 scalars
        n = float(maps["n"]) * B
        return 4.0 * n * T.nc, 4.0 * n * ((4 if YT is not None else 2) * T.nc + 5)
    return _timed("acl_tangent", cost, launch)


def acl_cotangent(Ct, YC, z, y, g, maps):
    """Adjoint of acl_tangent on the cotangent tensor ``Ct`` (in place on the modified rows); fills the modified rows of
    ``YC`` (cotangent of the coupler network's raw output; the caller zeroed it; None: not wanted)."""
    B = z.shape[0]
    z2 = z.view(B, -1)
    y2, y_b = _y_rows(y, B)
    _lib.check(_lib.load().cmf_acl_cotangent(_p(Ct.data), Ct.t_b, Ct.t_r, *_t3(YC), Ct.nc, _p(z2),
                                             z2.shape[1], _p(y2), y_b, _p(g), _p(maps["zi"]), _p(maps["si"]),
                                             _p(maps["ti"]), maps["n"], B, _stream()), "cmf_acl_cotangent")


def modified_rows(T, maps):
    """Compact copy (B, n_mod, nc) of the rows of ``T`` a coupling layer is about to update (kept for acl_cross_terms)."""
    out = Tangent(T.B, maps["n"], T.nc, T.layout, T.data.device)
    _lib.check(_lib.load().cmf_gather_tangent(_p(T.data), T.t_b, T.t_r, _p(out.data), out.t_b, out.t_r, _p(maps["zi"]), maps["n"],
                                              T.nc, T.B, _stream()), "cmf_gather_tangent")
    return out


def acl_primal_backward(dx, z, y, maps, dy, decode, dlj=None):
    """Primal backward of the coupling update, in place on ``dx`` (z-shaped); accumulates into ``dy`` (y-shaped).  ``z`` = the
    tensor the forward update read (decode: before the update; encode: the layer input)."""
    B = z.shape[0]
    d2, z2, y2 = dx.view(B, -1), z.view(B, -1), y.view(B, -1)
    _lib.check(_lib.load().cmf_acl_primal_backward(_p(d2), d2.shape[1], _p(z2), z2.shape[1], _p(y2), y2.shape[1], _p(dy), _p(maps["zi"]),
                                                   _p(maps["si"]), _p(maps["ti"]), maps["n"], B, int(decode), _p(dlj), _stream()),
               "cmf_acl_primal_backward")


def acl_cross_terms(Ct, V, YT, z, y, g, maps, dz, dy, dg):
    """Primal cotangents of the tangent update (training): column reductions accumulated into ``dz`` (like z), ``dy`` (like y:
    the log-scale entries) and ``dg`` (like g).  ``Ct`` must still hold the cotangent of the UPDATED rows: call this before
    ``acl_cotangent``.  ``V`` = ``modified_rows(T, maps)`` taken before ``acl_tangent``, ``YT`` = the network's raw tangent."""
    B = z.shape[0]
    z2, y2 = z.view(B, -1), y.view(B, -1)
    # YT None (network tangent identically zero): only the log-scale entries of dy receive a term; dz / dg are not touched
    _lib.check(_lib.load().cmf_acl_cross_terms(_p(Ct.data), Ct.t_b, Ct.t_r, _p(V.data), V.t_b, V.t_r, *_t3(YT),
                                               Ct.nc, _p(z2), z2.shape[1], _p(y2), y2.shape[1], _p(g), _p(maps["zi"]),
                                               _p(maps["si"]), _p(maps["ti"]), maps["n"], B, _p(dz), _p(dy), _p(dg), _stream()),
               "cmf_acl_cross_terms")


def relu_bits(act):
    """BitMask of [act > 0] for an activation tensor (B, C, H, W) (CMF_F_RELU_BITS layout)."""
    B, Cc = act.shape[0], act.shape[1]
    HW = act[0, 0].numel()
    m = BitMask(B, HW, Cc, act.device)
    _lib.check(_lib.load().cmf_relu_bits(_p(act.contiguous()), _p(m.data), B, Cc, HW, _stream()), "cmf_relu_bits")
    return m


def accumulate(dst, src):
    """dst += src (flat fp32 tensors of equal size; any length / alignment: cmf_accumulate has a scalar sweep for odd ones)."""
    _lib.check(_lib.load().cmf_accumulate(_p(dst), _p(src), min(dst.numel(), src.numel()), _stream()), "cmf_accumulate")


def accumulate_any(dst, src):
    """dst += src for flat fp32 tensors of any length (kept as a name: allocates nothing since round 4)."""
    assert src.numel() == dst.numel()
    accumulate(dst, src)


def stanh_backward(dy, dg, y, g, sw, sb, dsw=None, dsb=None):
    """ScaledTanh output stage backward: returns du for y = sw tanh(u) + sb, g = sw (1 - tanh^2) given the cotangents of y and g
    (``dg`` may be None); accumulates the parameter gradients into ``dsw`` / ``dsb`` (C floats each) when given."""
    B, Cc = y.shape[0], y.shape[1]
    HW = y[0, 0].numel()
    du = torch.empty_like(y)
    _lib.check(_lib.load().cmf_stanh_backward(_p(dy.contiguous()), _p(None if dg is None else dg.contiguous()), _p(y), _p(g),
                                              _p(sw.detach().reshape(-1).contiguous()), _p(sb.detach().reshape(-1).contiguous()),
                                              _p(du), _p(dsw), _p(dsb), B, Cc, HW, _stream()), "cmf_stanh_backward")
    return du


def channel_sum(t, t_np, t_c, t_px, np_, Cc, npx, nc, out, t_sl=16):
    """out[c] += sum of a tangent-layout tensor over samples, pixels and columns (bias gradients)."""
    _lib.check(_lib.load().cmf_channel_sum(_p(t), int(t_np), int(t_c), int(t_px), int(t_sl), int(np_), int(Cc), int(npx), int(nc),
                                           _p(out), _stream()), "cmf_channel_sum")


def channel_sum_batched(ts, t_np, t_c, t_px, np_, Cc, npx, nc, outs, t_sl=16):
    """``channel_sum`` for up to 16 tensors of one shape in one launch (lists of tensors and of the bias-gradient vectors)."""
    n = len(ts)
    assert n == len(outs) and 1 <= n <= _lib.WGRAD_MAX_BATCH
    arr = lambda xs: (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    _lib.check(_lib.load().cmf_channel_sum_batched(arr(ts), arr(outs), n, int(t_np), int(t_c), int(t_px), int(t_sl), int(np_), int(Cc), int(npx),
                                                   int(nc), _stream()), "cmf_channel_sum_batched")


#: widest Jacobian the head kernels take (column slots ceil16(d) <= 512); up to 128 the d x d matrix stays in LDS, wider runs
#: csrc/head_wide.hip
MAX_LATENT = 512
WIDE_NC = 128


def check_latent_width(d):
    """Raise before any launch when the Jacobian head cannot take d columns (sampling and latent extraction need no head)."""
    if not 1 <= int(d) <= MAX_LATENT:
        raise ValueError(f"latent_dimension = {int(d)}: the Jacobian head (Gram, Cholesky, Hutchinson kernels) supports "
                         f"1 <= latent_dimension <= {MAX_LATENT}")


class GramResult:
    """Outputs of ``gram_cholesky`` (all on the device).  ``gram_condition`` adds ``cond`` (B,) float32, ``flagged_count`` (1,)
    int32 and ``flagged_idx`` (B,) int32; a guarded evaluation that re-ran rows on its fallback kernels lists them in
    ``recomputed`` (int64).  Slots not filled are None."""
    __slots__ = ("jtj", "logdet", "l1_off", "l1_diag", "info", "fail", "attempts", "cond", "flagged_idx", "flagged_count",
                 "recomputed")

    def __init__(self):
        self.attempts = self.cond = self.flagged_idx = self.flagged_count = self.recomputed = None


def gram_cholesky(T, d, max_attempts=6, eps0=1e-6):
    """Fused Gram + Cholesky with the reference's whole-batch jitter retries enqueued back to back."""
    check_latent_width(d)
    lib = _lib.load()
    dev = T.data.device
    r = GramResult()
    r.jtj = torch.empty(T.B, d, d, dtype=torch.float32, device=dev)
    r.logdet = torch.empty(T.B, dtype=torch.float32, device=dev)
    r.l1_off = torch.empty(T.B, dtype=torch.float32, device=dev)
    r.l1_diag = torch.empty(T.B, dtype=torch.float32, device=dev)
    r.info = torch.empty(T.B, dtype=torch.int32, device=dev)
    r.fail = torch.empty(8, dtype=torch.int32, device=dev)
    launch = lambda: _lib.check(lib.cmf_gram_cholesky(_p(T.data), T.t_b, T.t_r, T.N, T.nc, d, T.B, _p(r.jtj), _p(r.logdet),
                                                      _p(r.l1_off), _p(r.l1_diag), _p(r.info), _p(r.fail), _stream()),
                                "cmf_gram_cholesky")

    def cost():
        if T.nc <= WIDE_NC:                        # 2 D d^2 (+ d^3/3) FLOP and (D NC + d^2 + 3) 4 B per sample
            return T.B * (2.0 * T.N * d * d + d ** 3 / 3.0), 4.0 * T.B * (T.N * T.nc + d * d + 3)
        # head_wide.hip: the lower-triangle tiles (half the products) and the factorisation's passes over jtj (l1 sums, panels,
        # trailing updates, restore)
        nt = -(-d // 64)
        return T.B * (2.0 * T.N * d * d + d ** 3 / 3.0), 4.0 * T.B * (nt * (nt + 1) // 2 * 2 * 64 * T.N + 4 * d * d + d ** 3 / 96.0)
    _timed("gram_cholesky" if T.nc <= WIDE_NC else "gram_cholesky_wide", cost, launch)
    cholesky_retries(r, d, max_attempts, eps0)
    return r


def cholesky_retries(r, d, max_attempts=6, eps0=1e-6):
    """Enqueue the whole-batch jitter retries 1 .. max_attempts-1 behind a factorisation (non_square.py:280-288): retry ``a``
    exits at once unless ``fail[a-1]`` is set, else adds eps0 * 10^(a-1) to every sample's diagonal IN PLACE and factorises again."""
    check_latent_width(d)
    lib = _lib.load()
    B = r.jtj.shape[0]
    for a in range(1, max_attempts):
        _lib.check(lib.cmf_cholesky_retry(_p(r.jtj), d, B, a, eps0, _p(r.logdet), _p(r.l1_diag), _p(r.info), _p(r.fail),
                                          _stream()), "cmf_cholesky_retry")


def gram_condition(r, d, threshold):
    """kappa_1 of every factorised Gram matrix in ``r`` (a GramResult of ``gram_cholesky``, after its retries) and the samples
    above ``threshold``: fills ``r.cond`` (B,) float32 (+inf where the factorisation failed), ``r.flagged_idx`` (B,) int32
    (ascending, -1 after the last) and ``r.flagged_count`` (1,) int32, all on the device, without synchronising."""
    check_latent_width(d)
    B, dev = r.jtj.shape[0], r.jtj.device
    r.cond = torch.empty(B, dtype=torch.float32, device=dev)
    r.flagged_idx = torch.empty(B, dtype=torch.int32, device=dev)
    r.flagged_count = torch.empty(1, dtype=torch.int32, device=dev)
    # 128 < d: the float64 factor lives in a torch-allocated workspace (a captured graph's pool serves it)
    ws = torch.empty(2 * B * d * d, dtype=torch.float32, device=dev) if d > WIDE_NC else None
    launch = lambda: _lib.check(_lib.load().cmf_gram_condition(_p(r.jtj), _p(r.info), d, B, float(threshold), _p(r.cond),
                                                               _p(r.flagged_idx), _p(r.flagged_count), _p(ws), _stream()),
                                "cmf_gram_condition")

    def cost():
        # float64 multiply-adds: factorisation d^3/6, triangular inverse d^3/6, |G^-1| column sums d^3/3 (2 FLOP each); bytes:
        # jtj in and cond out, plus for 128 < d the float64 matrix written once and re-read by every pass over it in L2 / HBM
        wide = 8.0 * (d * d + 2 * d ** 3 / 3.0) if d > WIDE_NC else 0.0
        return B * 2.0 * (2 * d ** 3 / 3.0), B * (4.0 * (d * d + 1) + wide) + 8.0 * B
    _timed("gram_condition", cost, launch)
    return r


#: samples one workgroup of ``metric_stats_accumulate`` sums before it writes a float64 partial (the fold adds the partials in chunk
#: order: with the batch size and d this constant fixes the summation order)
METRIC_STATS_CHUNK = 16


def metric_stats_state_size(d):
    """Doubles in the flat state of ``metric_stats_accumulate``: [S_G (d*d) | S_cos (d*d) | count | skipped]."""
    return 2 * int(d) * int(d) + 2


def metric_stats_workspace_size(B, d, sample_macs=True):
    """Doubles of workspace one ``metric_stats_accumulate`` call on (B, d, d) needs."""
    check_latent_width(d)
    n = _lib.load().cmf_metric_stats_ws(int(d), int(B), METRIC_STATS_CHUNK, int(bool(sample_macs)))
    _lib.check(min(n, 0), "cmf_metric_stats_ws")
    return n


def metric_stats_accumulate(jtj, state, workspace=None, sample_macs=None):
    """ADD the (B, d, d) float32 Gram matrices ``jtj`` to the flat float64 ``state`` (``metric_stats_state_size(d)`` doubles, on the
    device): running sums of G and of the column cosines G_ij / (n_i n_j), n_k = sqrt(G_kk) + 1e-8, and the numbers of samples
    counted and skipped (a sample counts iff its diagonal is finite and positive).  ``sample_macs`` (B,) float32, optional: each
    sample's mean |cos_ij| over i != j (NaN where skipped).  ``workspace``: float64, ``metric_stats_workspace_size`` doubles
    (allocated here when None).  Deterministic (no atomics); no synchronisation."""
    require_gpu(jtj, "jtj")
    if jtj.dim() != 3 or jtj.shape[1] != jtj.shape[2] or not jtj.is_contiguous():
        raise ValueError(f"jtj must be a contiguous (B, d, d) tensor, got {tuple(jtj.shape)}")
    B, d = jtj.shape[0], jtj.shape[1]
    check_latent_width(d)
    if state.dtype != torch.float64 or state.device != jtj.device or not state.is_contiguous() or \
            state.numel() != metric_stats_state_size(d):
        raise ValueError(f"state must be {metric_stats_state_size(d)} contiguous float64 values on {jtj.device}")
    if sample_macs is not None and (sample_macs.dtype != torch.float32 or sample_macs.device != jtj.device
                                    or not sample_macs.is_contiguous() or sample_macs.numel() != B):
        raise ValueError(f"sample_macs must be {B} contiguous float32 values on {jtj.device}")
    if B == 0:
        return state
    need = metric_stats_workspace_size(B, d, sample_macs is not None)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=jtj.device)
    elif workspace.dtype != torch.float64 or workspace.device != jtj.device or not workspace.is_contiguous() or \
            workspace.numel() < need:
        raise ValueError(f"workspace must be at least {need} contiguous float64 values on {jtj.device}")
    launch = lambda: _lib.check(_lib.load().cmf_metric_stats_accumulate(
        _p(jtj), d, B, METRIC_STATS_CHUNK, _p(state), _p(workspace), workspace.numel(), _p(sample_macs), _stream()),
        "cmf_metric_stats_accumulate")

    def cost():
        # per element one conversion, two multiplies, two adds and an abs in float64; bytes: jtj in, the chunk partials out and in
        n_chunks = -(-B // METRIC_STATS_CHUNK)
        return 6.0 * B * d * d, 4.0 * B * d * d + 16.0 * (n_chunks + 1) * metric_stats_state_size(d)
    _timed("metric_stats", cost, launch)
    return state


# the argument rules of the head and manifold wrappers below, each stated once; all raise ValueError before any launch


def _check_on_gpu(name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be on the GPU, got {getattr(t, 'device', type(t).__name__)} (there is no CPU fallback)")


def _check_tensor(name, t, dtype, want=None, fits=None, device=None):
    """``t`` is a tensor on the GPU of ``dtype`` and, with ``want`` -- the words for its shape --, contiguous, of a shape that
    ``fits(t)`` accepts and, where one is given, on ``device``."""
    _check_on_gpu(name, t)
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {str(dtype).split('.')[1]}, got {t.dtype}")
    if want is not None and not (fits(t) and t.is_contiguous() and (device is None or t.device == device)):
        on, on_t = ("", "") if device is None else (f" on {device}", f" on {t.device}")
        raise ValueError(f"{name} must be a contiguous {want} tensor{on}, got {tuple(t.shape)}{on_t}"
                         f"{'' if t.is_contiguous() else ' (not contiguous)'}")


def _check_width(d, kernel, limit):
    if not 1 <= d <= limit:
        raise ValueError(f"d = {d}: {kernel} 1 <= d <= {limit}")


def _gram_stack(jtj, rows, kernel, limit):
    """``jtj`` is a contiguous float32 (``rows``, d, d) stack on the GPU, no wider than ``kernel`` takes: returns (its rows, d)."""
    _check_tensor("jtj", jtj, torch.float32, f"({rows}, d, d)", lambda t: t.dim() == 3 and t.shape[1] == t.shape[2])
    _check_width(jtj.shape[1], kernel, limit)
    return jtj.shape[0], jtj.shape[1]


def _check_tangent(T):
    if not isinstance(T, Tangent):
        raise ValueError(f"T must be an engine.Tangent, got {type(T).__name__}")


def _whole_curves(points, rows, name, least=3):
    """The number of curves of ``points`` points in the ``rows`` curve-major samples of ``name``."""
    if points < least or rows % points:
        raise ValueError(f"points = {points}: a curve needs points >= {least}, and the {rows} samples of {name} must be whole curves")
    return rows // points


def _check_damping(damping, rows, dev):
    if not isinstance(damping, torch.Tensor) or damping.dtype != torch.float64 or damping.device != dev or \
            damping.shape != (rows,) or not damping.is_contiguous():
        raise ValueError(f"damping must be {rows} contiguous float64 values on {dev}")


#: widest Gram matrix ``gram_spectrum`` takes: the float64 matrix of a sample lives in LDS (csrc/gram_spectrum.hip)
SPECTRUM_MAX_WIDTH = 128


class SpectrumResult:
    """Outputs of ``gram_spectrum`` (all on the device): ``eigenvalues`` (B, d) float64 ascending, ``vectors`` (B, d, d) float64
    (column k belongs to eigenvalue k) or None, ``sweeps`` (B,) int32, ``info`` (B,) int32 (0 converged, 1 sweep cap reached,
    2 non-finite input: NaN outputs)."""
    __slots__ = ("eigenvalues", "vectors", "sweeps", "info")


def gram_spectrum(jtj, vectors=False):
    """Eigenvalues (and, with ``vectors``, eigenvectors) of every (d, d) matrix of ``jtj`` (B, d, d) float32, whose lower
    triangles are read: float64 cyclic Jacobi, one workgroup per sample.  Deterministic per sample; enqueues one
    launch, no synchronisation."""
    B, d = _gram_stack(jtj, "B", "the spectrum kernel supports", SPECTRUM_MAX_WIDTH)
    r = SpectrumResult()
    r.eigenvalues = torch.empty(B, d, dtype=torch.float64, device=jtj.device)
    r.vectors = torch.empty(B, d, d, dtype=torch.float64, device=jtj.device) if vectors else None
    r.sweeps = torch.empty(B, dtype=torch.int32, device=jtj.device)
    r.info = torch.empty(B, dtype=torch.int32, device=jtj.device)
    if B == 0:
        return r
    launch = lambda: _lib.check(_lib.load().cmf_gram_spectrum(_p(jtj), d, B, _p(r.eigenvalues), _p(r.vectors), _p(r.sweeps),
                                                              _p(r.info), _stream()), "cmf_gram_spectrum")
    # a nominal 10 sweeps of d (d - 1) / 2 rotations, each 6 float64 FLOP on 2 d entry pairs of A (+ d of V); bytes: jtj in,
    # the outputs out (the iteration itself runs in LDS)
    _timed("gram_spectrum", lambda: (B * 10.0 * (d * (d - 1) / 2) * 6.0 * (3 if vectors else 2) * d,
                                     B * (4.0 * d * d + 8.0 * d + (8.0 * d * d if vectors else 0.0) + 8.0)), launch)
    return r


#: widest Jacobian ``gauss_newton_step`` takes: the float64 matrix of a sample lives in LDS (csrc/gn_step.hip)
PROJECT_MAX_WIDTH = 128


class GaussNewtonResult:
    """Outputs of ``gauss_newton_step`` (all on the device): ``grad`` (B, d) float64 = J^T (x - x_hat), ``delta`` (B, d) float64 =
    (G + lambda diag G)^-1 grad, ``stats`` (B, 4) float64 = [||x - x_hat||^2, grad^T delta, delta^T G delta, max |grad_k|],
    ``info`` (B,) int32 (0 ok, 1 non-positive pivot: delta and stats[:, 1:3] NaN, 2 non-finite input: everything NaN)."""
    __slots__ = ("grad", "delta", "stats", "info")


def _residual_pair(x, xhat):
    """The checks ``gauss_newton_step`` and ``residual_sqnorm`` share; returns (B, elements per sample)."""
    for name, v in (("x", x), ("xhat", xhat)):
        _check_tensor(name, v, torch.float32, "(B, ...)", lambda t: t.dim() >= 2)
    if x.shape != xhat.shape or x.device != xhat.device:
        raise ValueError(f"x {tuple(x.shape)} on {x.device} and xhat {tuple(xhat.shape)} on {xhat.device} must agree")
    B = x.shape[0]
    n = x.numel() // B if B else int(np.prod(x.shape[1:]))
    if n < 1:
        raise ValueError(f"x must have at least one element per sample, got {tuple(x.shape)}")
    return B, n


def residual_sqnorm(x, xhat):
    """||x_b - xhat_b||^2 per sample in float64, by the residual-only mode of the Gauss-Newton step kernel (the same arithmetic,
    bit for bit, as ``gauss_newton_step(...).stats[:, 0]``): returns ((B,) float64, info (B,) int32 -- 0, or 2 with a NaN norm
    for a non-finite input).  One launch, no synchronisation."""
    B, n = _residual_pair(x, xhat)
    stats = torch.empty(B, 4, dtype=torch.float64, device=x.device)
    info = torch.empty(B, dtype=torch.int32, device=x.device)
    if B == 0:
        return stats[:, 0], info
    launch = lambda: _lib.check(_lib.load().cmf_gauss_newton_step(None, 0, 0, n, 0, 0, B, None, _p(x), _p(xhat), None, None, None,
                                                                  _p(stats), _p(info), _stream()), "cmf_gauss_newton_step")
    # a subtraction, a multiply and an add per element; x and xhat in
    _timed("residual_sqnorm", lambda: (3.0 * B * n, B * (8.0 * n + 12.0)), launch)
    return stats[:, 0], info


def gauss_newton_step(T, jtj, x, xhat, damping):
    """One damped Gauss-Newton step per sample: from the Jacobian stack ``T`` of a decode sweep, its Gram matrix
    ``jtj`` (B, d, d) float32 (one ``gram_cholesky`` attempt; the lower triangles are read), the head-space input ``x`` and the
    reconstruction ``xhat`` (B, ...) float32 and ``damping`` (B,) float64 >= 0, in float64: grad = J^T (x - xhat) and delta =
    (G + damping diag G)^-1 grad.  Returns a ``GaussNewtonResult``.  Deterministic per sample; one launch, no synchronisation."""
    _check_tangent(T)
    B, n = _residual_pair(x, xhat)
    dev = x.device
    _, d = _gram_stack(jtj, "B", "the Gauss-Newton step kernel supports", PROJECT_MAX_WIDTH)
    if T.B != B or T.N != n or T.nc % 16 or T.nc < d or jtj.shape[0] != B or T.data.device != dev or jtj.device != dev:
        raise ValueError(f"T (B = {T.B}, N = {T.N}, nc = {T.nc}) on {T.data.device} must hold d = {d} <= nc columns, nc % 16 == 0, "
                         f"for the {B} samples of {n} elements of x on {dev}, like jtj {tuple(jtj.shape)} on {jtj.device}")
    _check_damping(damping, B, dev)
    r = GaussNewtonResult()
    r.grad = torch.empty(B, d, dtype=torch.float64, device=dev)
    r.delta = torch.empty(B, d, dtype=torch.float64, device=dev)
    r.stats = torch.empty(B, 4, dtype=torch.float64, device=dev)
    r.info = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return r
    launch = lambda: _lib.check(_lib.load().cmf_gauss_newton_step(_p(T.data), T.t_b, T.t_r, n, T.nc, d, B, _p(jtj), _p(x), _p(xhat),
                                                                  _p(damping), _p(r.grad), _p(r.delta), _p(r.stats), _p(r.info),
                                                                  _stream()), "cmf_gauss_newton_step")

    def cost():
        # float64: J^T r 2 D d, the elimination d^3 / 3 with the two substitutions 2 d^2, the residual 3 D and the two forms
        # 3 d^2 / 2 + 2 d; bytes: the live quarter-rows of J, x and xhat twice (L2 the second time), the triangle of G twice, the outputs
        ncl = min(T.nc, -(-d // 4) * 4)
        return (B * (2.0 * n * d + d ** 3 / 3.0 + 3.5 * d * d + 3.0 * n + 2.0 * d),
                B * (4.0 * n * ncl + 16.0 * n + 4.0 * d * (d + 1) + 16.0 * d + 44.0))
    _timed("gauss_newton_step", cost, launch)
    return r


class WeightedGaussNewtonResult(GaussNewtonResult):
    """Outputs of ``weighted_gauss_newton_step``: the fields of ``GaussNewtonResult`` for the weighted system -- ``grad`` = J^T (w o
    (x - x_hat)), ``delta`` = (G_w + lambda diag G_w)^-1 grad, ``stats`` = [sum w r^2, grad^T delta, delta^T G_w delta, max |grad_k|]
    -- plus ``gram`` (B, d, d) float32 = G_w = J^T diag(w) J, symmetric bit for bit.  ``info``: 0 ok, 1 non-positive pivot (delta and
    stats[:, 1:3] NaN), 2 a negative or non-finite weight or a non-finite value in a row with w > 0 (everything NaN)."""
    __slots__ = ("gram",)


def _weighted_triple(w, x, xhat):
    """The checks ``weighted_gauss_newton_step`` and ``weighted_residual_sqnorm`` share; returns (B, elements per sample)."""
    B, n = _residual_pair(x, xhat)
    _check_tensor("w", w, torch.float32, f"({B}, ...) of {n} elements per sample", lambda t: t.dim() >= 2 and t.shape[0] == B and
                  t.numel() == B * n, x.device)
    return B, n


def weighted_residual_sqnorm(w, x, xhat):
    """sum_i w_bi (x_bi - xhat_bi)^2 per sample in float64, by the cost-only mode of the weighted Gauss-Newton step kernel (the
    same arithmetic, bit for bit, as ``weighted_gauss_newton_step(...).stats[:, 0]``); elements with w == 0 are not read.  Returns
    ((B,) float64, info (B,) int32 -- 0, or 2 with a NaN cost for a negative or non-finite weight or a non-finite value where
    w > 0).  One launch, no synchronisation."""
    B, n = _weighted_triple(w, x, xhat)
    stats = torch.empty(B, 4, dtype=torch.float64, device=x.device)
    info = torch.empty(B, dtype=torch.int32, device=x.device)
    if B == 0:
        return stats[:, 0], info
    launch = lambda: _lib.check(_lib.load().cmf_weighted_gauss_newton_step(
        None, 0, 0, n, 0, 0, B, _p(w), _p(x), _p(xhat), None, None, None, None, _p(stats), _p(info), _stream()),
        "cmf_weighted_gauss_newton_step")

    def cost():
        live = float((w > 0).sum())                                   # a host look: under a timer only
        return 4.0 * live, 4.0 * B * n + 8.0 * live + 12.0 * B
    _timed("weighted_residual_sqnorm", cost, launch)
    return stats[:, 0], info


def weighted_gauss_newton_step(T, w, x, xhat, damping, d=None):
    """One damped, weighted Gauss-Newton step per sample: from the Jacobian stack ``T`` of a decode sweep, of which
    the first ``d`` columns are J (default: all ``T.nc``; there is no Gram matrix among the arguments to tell the width), the
    weights ``w`` >= 0, the head-space input ``x`` and the reconstruction ``xhat`` (B, ...) float32 and ``damping`` (B,) float64
    >= 0: gram = J^T diag(w) J in float32 and, in float64, grad = J^T (w o (x - xhat)) and delta = (gram + damping diag gram)^-1
    grad -- J is read once, and only its rows with w > 0.  Returns a ``WeightedGaussNewtonResult``.  Deterministic per sample;
    one launch, no synchronisation."""
    _check_tangent(T)
    B, n = _weighted_triple(w, x, xhat)
    dev = x.device
    d = T.nc if d is None else int(d)
    _check_width(d, "the weighted Gauss-Newton step kernel supports", PROJECT_MAX_WIDTH)
    if T.B != B or T.N != n or T.nc % 16 or T.nc < d or T.data.device != dev:
        raise ValueError(f"T (B = {T.B}, N = {T.N}, nc = {T.nc}) on {T.data.device} must hold d = {d} <= nc columns, nc % 16 == 0, "
                         f"for the {B} samples of {n} elements of x on {dev}")
    _check_damping(damping, B, dev)
    r = WeightedGaussNewtonResult()
    r.gram = torch.empty(B, d, d, dtype=torch.float32, device=dev)
    r.grad = torch.empty(B, d, dtype=torch.float64, device=dev)
    r.delta = torch.empty(B, d, dtype=torch.float64, device=dev)
    r.stats = torch.empty(B, 4, dtype=torch.float64, device=dev)
    r.info = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return r
    launch = lambda: _lib.check(_lib.load().cmf_weighted_gauss_newton_step(
        _p(T.data), T.t_b, T.t_r, n, T.nc, d, B, _p(w), _p(x), _p(xhat), _p(damping), _p(r.gram), _p(r.grad), _p(r.delta),
        _p(r.stats), _p(r.info), _stream()), "cmf_weighted_gauss_newton_step")

    def cost():
        # per live row: the lower tile triangle of the Gram MFMAs (2 flop per product, nt (nt + 1) / 2 tiles of 256), the float64
        # J^T (w r) 2 d and the cost 4; per sample the elimination as in gauss_newton_step.  Bytes: w once; per live row x, xhat
        # and the 16-column tiles of J that hold the first d columns ONCE; gram out and its triangle back twice, the outputs
        live = float((w > 0).sum())                                   # a host look: under a timer only
        nt = -(-d // 16)
        return (live * (2.0 * 256.0 * nt * (nt + 1) / 2 + 2.0 * d + 4.0) + B * (d ** 3 / 3.0 + 3.5 * d * d + 2.0 * d),
                4.0 * B * n + live * (8.0 + 64.0 * nt) + B * (4.0 * d * d + 4.0 * d * (d + 1) + 16.0 * d + 44.0))
    _timed("weighted_gauss_newton_step", cost, launch)
    return r


#: the losses ``robust_weights`` takes, in the kernel's numbering
ROBUST_LOSSES = {"huber": 0, "tukey": 1}
#: radix passes of the exact median: eight bytes of a float64 key (csrc/robust_weights.hip)
ROBUST_SELECT_PASSES = 8


class RobustWeightsResult:
    """Outputs of ``robust_weights`` (all on the device): ``w`` x's shape float32 = prior * omega (None with ``weights_out=False``),
    ``scale`` (B,) float64 = s, ``cost`` (B,) float64 = 2 s^2 sum prior rho(r / s), ``used`` (B,) float64 = the count of elements
    with prior > 0 (a whole number), ``effective`` (B,) float64 = sum omega over them, ``info`` (B,) int32 (0 ok; 2 a negative or
    non-finite prior or a non-finite value at a used element: everything NaN; 3 a scale that is not finite or not > 0: everything
    NaN but ``scale``).  The four float64 fields are views of one (B, 4) tensor, ``stats``."""
    __slots__ = ("w", "stats", "scale", "cost", "used", "effective", "info")


def robust_weights(x, xhat, loss, tuning, prior=None, scale=None, weights_out=True):
    """The robust scale, IRLS weights and robust cost of the residual x - xhat per sample, in float64: s = ``scale``
    (B,) float64 where given, else 1.4826 x the exact lower median of |x - xhat| over the elements with ``prior`` > 0 (``prior``
    None: all, weight 1); w = prior * omega((x - xhat) / s) for ``loss`` "huber" or "tukey" with the constant ``tuning`` > 0.
    Elements with prior == 0 are not read.  Returns a ``RobustWeightsResult``.  Deterministic per sample; one launch, no
    synchronisation."""
    B, n = _residual_pair(x, xhat)
    dev = x.device
    if prior is not None:                                             # the rule of ``_weighted_triple``, under this argument's name
        _check_tensor("prior", prior, torch.float32, f"({B}, ...) of {n} elements per sample", lambda t: t.dim() >= 2 and
                      t.shape[0] == B and t.numel() == B * n, dev)
    if loss not in ROBUST_LOSSES:
        raise ValueError(f"loss must be one of {sorted(ROBUST_LOSSES)}, got {loss!r}")
    if not float(tuning) > 0:
        raise ValueError(f"tuning must be > 0, got {tuning}")
    if scale is not None:
        _check_tensor("scale", scale, torch.float64, f"({B},)", lambda t: tuple(t.shape) == (B,), dev)
    r = RobustWeightsResult()
    r.w = torch.empty_like(x) if weights_out else None
    r.stats = torch.empty(B, 4, dtype=torch.float64, device=dev)
    r.scale, r.cost, r.used, r.effective = (r.stats[:, k] for k in range(4))
    r.info = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return r
    launch = lambda: _lib.check(_lib.load().cmf_robust_weights(
        _p(x), _p(xhat), _p(prior), n, B, ROBUST_LOSSES[loss], float(tuning), _p(scale), _p(r.w), _p(r.stats), _p(r.info), _stream()),
        "cmf_robust_weights")

    def cost():
        # per used element and pass: the float64 difference and its key (3); the weights pass a division and about ten more.
        # Bytes: prior (where there is one), x and xhat once per pass -- the validating pass, the select passes after the first
        # (it shares the validating pass) and the weights pass; HBM sees them once, the rest is L2 --, w out, the outputs
        passes = 2 + (0 if scale is not None else ROBUST_SELECT_PASSES - 1)
        used = float(B * n) if prior is None else float((prior > 0).sum())     # a host look: under a timer only
        return (used * (3.0 * passes + 12.0),
                passes * ((0.0 if prior is None else 4.0 * B * n) + 8.0 * used) + (4.0 * B * n if weights_out else 0.0) + 36.0 * B)
    _timed("robust_weights", cost, launch)
    return r


class LeverageResult:
    """Outputs of ``tangent_leverage`` (all on the device): ``cov`` (B, d, d) float64 = gram^-1, symmetric bit for bit, ``lev``
    (B, N) float64 = j_i^T gram^-1 j_i >= +0.0 per row of J, ``stats`` (B, 2) float64 = [sum_i lev_i, max_i lev_i] (both None
    with ``rows=False``), ``info`` (B,) int32 (0 ok, 1 non-positive pivot, 2 non-finite input: every output NaN in both cases)."""
    __slots__ = ("cov", "lev", "stats", "info")


def tangent_leverage(T, gram, rows=True):
    """The covariance of a Gauss-Newton fit and its image on every row of J, per sample in float64: from the
    Jacobian stack ``T`` of a decode sweep and ``gram`` (B, d, d) float32 -- any normal matrix a step kernel consumes: the ``jtj``
    of one ``gram_cholesky`` attempt, the ``gram`` of ``weighted_gauss_newton_step``, or the Gram matrix of a measured stack; the
    lower triangles are read --, cov = gram^-1 and lev_i = j_i^T cov j_i over the first d columns of ``T``.  With ``rows=False``
    only ``cov`` and ``info`` are computed (the same bits) and ``T`` is not read.  Returns a ``LeverageResult``.  Deterministic
    per sample; one launch, no synchronisation."""
    _check_tangent(T)
    B, d = _gram_stack(gram, "B", "the leverage kernel supports", PROJECT_MAX_WIDTH)
    dev = gram.device
    if T.B != B or T.nc % 16 or T.nc < d or T.data.device != dev:
        raise ValueError(f"T (B = {T.B}, N = {T.N}, nc = {T.nc}) on {T.data.device} must hold d = {d} <= nc columns, nc % 16 == 0, "
                         f"for the {B} samples of jtj {tuple(gram.shape)} on {dev}")
    n = T.N
    r = LeverageResult()
    r.cov = torch.empty(B, d, d, dtype=torch.float64, device=dev)
    r.lev = torch.empty(B, n, dtype=torch.float64, device=dev) if rows else None
    r.stats = torch.empty(B, 2, dtype=torch.float64, device=dev) if rows else None
    r.info = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return r
    if rows:
        launch = lambda: _lib.check(_lib.load().cmf_tangent_leverage(_p(T.data), T.t_b, T.t_r, n, T.nc, d, B, _p(gram), _p(r.cov),
                                                                     _p(r.lev), _p(r.stats), _p(r.info), _stream()),
                                    "cmf_tangent_leverage")
    else:
        launch = lambda: _lib.check(_lib.load().cmf_tangent_leverage(None, 0, 0, 0, 0, d, B, _p(gram), _p(r.cov), None, None,
                                                                     _p(r.info), _stream()), "cmf_tangent_leverage")

    def cost():
        # float64: the elimination d^3 / 3, the inverse of the unit factor d^3 / 3, cov d^3 / 2 (three operations per term of a
        # d^3 / 6 sum) and, per row, d^2 / 2 multiply-adds with 3 d for the squares; bytes: the live quarter-rows of J once, the
        # triangle of gram in, cov and lev out, stats and info
        ncl = min(T.nc, -(-d // 4) * 4)
        nr = n if rows else 0
        return (B * (7.0 * d ** 3 / 6.0 + nr * (1.0 * d * d + 3.0 * d)),
                B * (4.0 * nr * ncl + 2.0 * d * (d + 1) + 8.0 * d * d + 8.0 * nr + (16.0 if rows else 0.0) + 4.0))
    _timed("tangent_leverage", cost, launch)
    return r


def _operator_pair(a, xhat):
    """The checks ``operator_apply`` and ``operator_image`` share; returns (B, M, D)."""
    _check_tensor("a", a, torch.float32, "(M, D)", lambda t: t.dim() == 2 and t.shape[0] >= 1 and t.shape[1] >= 1)
    D = a.shape[1]
    _check_tensor("xhat", xhat, torch.float32, f"(B, ...) of {D} elements per sample",
                  lambda t: t.dim() >= 2 and int(np.prod(t.shape[1:])) == D, a.device)
    return xhat.shape[0], a.shape[0], D


def _operator_wrapper(wrapper):
    """The fused pre-head triple (wa, wc, logit) as ``cmf_operator_apply_wrapped`` takes it: what it would refuse is said here."""
    try:
        wa, wc, logit = wrapper
        wa, wc = float(wa), float(wc)
    except (TypeError, ValueError):
        raise ValueError(f"wrapper must be a (wa, wc, logit) triple, got {wrapper!r}") from None
    if wa == 0.0 or not math.isfinite(wa) or not math.isfinite(wc) or logit not in (0, 1, False, True):
        raise ValueError(f"wrapper needs a finite wa != 0, a finite wc and logit in (0, 1), got {wrapper!r}")
    return wa, wc, int(logit)


#: what ``operator_image`` and ``operator_apply`` hand the shared code in place of a wrapper
_PLAIN = object()


def _operator_image(name, a, xhat, wrapper):
    """``operator_image`` (``wrapper`` is _PLAIN) and ``operator_image_wrapped``: the image-only mode of either entry point."""
    B, M, D = _operator_pair(a, xhat)
    w = None if wrapper is _PLAIN else _operator_wrapper(wrapper)
    yhat = torch.empty(B, M, dtype=torch.float32, device=a.device)
    if B == 0:
        return yhat
    if w is None:
        launch = lambda: _lib.check(_lib.load().cmf_operator_apply(_p(a), M, D, None, 0, 0, 0, B, _p(xhat), None, 0, 0, _p(yhat),
                                                                   _stream()), "cmf_operator_apply")
    else:
        launch = lambda: _lib.check(_lib.load().cmf_operator_apply_wrapped(_p(a), M, D, None, 0, 0, 0, B, _p(xhat), *w, None, None,
                                                                           0, 0, _p(yhat), _stream()), "cmf_operator_apply_wrapped")
    # a float64 multiply and add per element of a and sample; bytes: xhat in, yhat out, a once (every further read is L2's)
    _timed(name, lambda: (2.0 * B * M * D, 4.0 * (B * (D + M) + M * D)), launch)
    return yhat


def _operator_apply(name, T, a, xhat, wrapper, scale):
    """``operator_apply`` (``wrapper`` is _PLAIN) and ``operator_apply_wrapped``: the full mode of either entry point."""
    _check_tangent(T)
    B, M, D = _operator_pair(a, xhat)
    w = None if wrapper is _PLAIN else _operator_wrapper(wrapper)
    dev = a.device
    if T.B != B or T.N != D or T.nc % 16 or not 16 <= T.nc <= 512 or T.data.device != dev:
        raise ValueError(f"T (B = {T.B}, N = {T.N}, nc = {T.nc}) on {T.data.device} must hold 16 <= nc <= 512 columns, nc % 16 == 0, "
                         f"for the {B} samples of {D} elements of xhat on {dev}")
    if w is not None:
        if scale is None:
            scale = torch.empty(B, D, dtype=torch.float32, device=dev)
        else:
            _check_tensor("scale", scale, torch.float32, f"({B}, {D})", lambda t: tuple(t.shape) == (B, D), dev)
    K = Tangent(B, M, T.nc, T.layout, dev)
    yhat = torch.empty(B, M, dtype=torch.float32, device=dev)
    if B == 0:
        return K, yhat, scale
    if w is None:
        launch = lambda: _lib.check(_lib.load().cmf_operator_apply(_p(a), M, D, _p(T.data), T.t_b, T.t_r, T.nc, B, _p(xhat),
                                                                   _p(K.data), K.t_b, K.t_r, _p(yhat), _stream()), "cmf_operator_apply")
    else:
        launch = lambda: _lib.check(_lib.load().cmf_operator_apply_wrapped(
            _p(a), M, D, _p(T.data), T.t_b, T.t_r, T.nc, B, _p(xhat), *w, _p(scale), _p(K.data), K.t_b, K.t_r, _p(yhat), _stream()),
            "cmf_operator_apply_wrapped")

    def cost():
        # fp32 MFMA: 2 M D per column over the whole row tiles of a (16 rows each), plus the image's 2 M D in float64; bytes: J
        # once per group of 256 rows of a, K out, xhat in, yhat out, a once (its re-reads by every workgroup are L2's).  Wrapped:
        # one more multiply per element of J and pass; xhat once more for scale, scale out and in once per pass
        tiles, passes = -(-M // 16), -(-M // 256)
        more = (0.0, 0.0) if w is None else (1.0 * B * passes * D * T.nc, 4.0 * B * D * (2 + passes))
        return (B * (2.0 * 16 * tiles * D * T.nc + 2.0 * M * D) + more[0],
                4.0 * (B * (passes * D * T.nc + M * T.nc + D + M) + M * D) + more[1])
    _timed(name, cost, launch)
    return K, yhat, scale


def operator_image(a, xhat):
    """yhat (B, M) float32 = a xhat per sample for the operator ``a`` (M, D) float32 and ``xhat`` (B, ...) float32 of D elements
    per sample, by the image-only mode of the operator kernel (the same arithmetic, bit for bit, as
    ``operator_apply(...)[1]``): every sum in float64 in a fixed order, rounded once.  One launch, no synchronisation."""
    return _operator_image("operator_image", a, xhat, _PLAIN)


def operator_apply(T, a, xhat):
    """The linear operator ``a`` (M, D) float32 carried through a decode sweep: from the Jacobian stack ``T`` of D
    rows and ``xhat`` (B, ...) float32 of D elements per sample, (K, yhat) with K = a J per sample -- a ``Tangent`` of M rows in
    T's layout with T's nc columns (fp32 MFMA, fp32 accumulation; column c of K depends on column c of T alone) -- and yhat (B, M)
    float32 = a xhat (float64 sums).  What ``gram_cholesky`` and ``gauss_newton_step`` take in place of (T, xhat) for the recovery
    min_z ||y - a g(z)||^2.  Deterministic per sample; no synchronisation."""
    return _operator_apply("operator_apply", T, a, xhat, _PLAIN, None)[:2]


def operator_image_wrapped(a, xhat, wrapper):
    """``operator_image`` in data space: yhat (B, M) float32 = a u(xhat) with u the inverse of the fused pre-head
    wrapper v = [logit](wa x + wc), ``wrapper`` = (wa, wc, logit), evaluated in float64 in front of the float64 sum.  The same
    bits as ``operator_apply_wrapped(...)[1]``; with (1, 0, False), ``operator_image``'s.  One launch, no synchronisation."""
    return _operator_image("operator_image_wrapped", a, xhat, wrapper)


def operator_apply_wrapped(T, a, xhat, wrapper, scale=None):
    """``operator_apply`` in data space, for an operator that acts on the density's input behind the fused pre-head
    wrapper v = [logit](wa x + wc), ``wrapper`` = (wa, wc, logit): (K, yhat, scale) with scale (B, D) float32 = du/dv at xhat
    (float64, rounded once), K = a diag(scale) J per sample -- every element of J times its row's scale value in fp32, then
    ``operator_apply``'s MFMAs -- and yhat = a u(xhat).  ``scale``: an optional (B, D) float32 buffer to write into, for a loop
    that calls this every step; allocated otherwise.  With (1, 0, False), scale is 1 and (K, yhat) are ``operator_apply``'s bits.
    Deterministic per sample; no synchronisation."""
    return _operator_apply("operator_apply_wrapped", T, a, xhat, wrapper, scale)

#: widest Jacobian ``cross_gram`` / ``curve_step`` take (csrc/curve_step.hip: the elimination window of a curve lives in LDS up to
#: d = 64 and in a workspace slice up to d = 128)
GEODESIC_MAX_WIDTH = 128


class CurveStepResult:
    """Outputs of ``curve_step`` (all on the device, float64 unless noted) for curves of P points, N = P - 1 segments and M = P - 2
    interior points: ``grad`` and ``delta`` (curves, M, d), ``stats`` (curves, 4) = [sum_i ||r_i||^2, g^T delta, delta^T H delta,
    max |g|], ``seg2`` (curves, N) = ||r_i||^2, ``info`` (curves,) int32 (0 ok, 1 non-positive pivot: delta and stats[:, 1:3] NaN,
    2 non-finite input: everything NaN)."""
    __slots__ = ("grad", "delta", "stats", "seg2", "info")


def _curve_points(xhat, points):
    """The checks ``curve_step`` and ``curve_energy`` share; returns (curves, elements per point)."""
    _check_tensor("xhat", xhat, torch.float32, "(curves * points, ...)", lambda t: t.dim() >= 2)
    curves = _whole_curves(int(points), xhat.shape[0], "xhat")
    n = int(np.prod(xhat.shape[1:]))
    if n < 1:
        raise ValueError(f"xhat must have at least one element per point, got {tuple(xhat.shape)}")
    return curves, n


def _curve_tangent(T, d, points):
    _check_tangent(T)
    _check_on_gpu("T", T.data)
    _check_width(int(d), "the curve kernels support", GEODESIC_MAX_WIDTH)
    _whole_curves(int(points), T.B, "T")
    if T.nc % 16 or T.nc < d or T.nc > GEODESIC_MAX_WIDTH:
        raise ValueError(f"T (nc = {T.nc}) must hold d = {int(d)} <= nc <= {GEODESIC_MAX_WIDTH} columns, nc % 16 == 0")


def cross_gram(T, d, points):
    """The cross-Gram matrices of neighbouring interior points of curve-major curves: ``T`` holds curves * points
    samples, the result is (curves, points - 3, d, d) float32 with [c, i - 1] = J_{c,i}^T J_{c,i+1}, i = 1 .. points - 3.  fp32 MFMA,
    deterministic per pair; one launch, no synchronisation."""
    _curve_tangent(T, d, points)
    d, points = int(d), int(points)
    curves = T.B // points
    out = torch.empty(curves, points - 3, d, d, dtype=torch.float32, device=T.data.device)
    if out.numel() == 0:
        return out
    launch = lambda: _lib.check(_lib.load().cmf_cross_gram(_p(T.data), T.t_b, T.t_r, T.N, T.nc, d, points, curves, _p(out), _stream()),
                                "cmf_cross_gram")

    def cost():                                    # 2 D d^2 FLOP per pair; both panels in, the block out
        pairs = curves * (points - 3)
        return pairs * 2.0 * T.N * d * d, 4.0 * pairs * (2 * T.N * T.nc + d * d)
    _timed("cross_gram", cost, launch)
    return out


def curve_energy(xhat, points):
    """||xhat_{i+1} - xhat_i||^2 per segment of curve-major curves in float64, by the energy-only mode of the curve step kernel (the
    same arithmetic, bit for bit, as ``curve_step(...).seg2`` and ``.stats[:, 0]``): returns (seg2 (curves, points - 1) float64, their
    sum (curves,) float64, info (curves,) int32 -- 0, or 2 with NaN outputs for a non-finite input).  One launch, no
    synchronisation."""
    curves, n = _curve_points(xhat, points)
    points = int(points)
    seg2 = torch.empty(curves, points - 1, dtype=torch.float64, device=xhat.device)
    stats = torch.empty(curves, 4, dtype=torch.float64, device=xhat.device)
    info = torch.empty(curves, dtype=torch.int32, device=xhat.device)
    if curves == 0:
        return seg2, stats[:, 0], info
    launch = lambda: _lib.check(_lib.load().cmf_curve_step(None, 0, 0, n, 0, 0, points, curves, None, None, _p(xhat), None, None, None,
                                                           _p(stats), _p(seg2), _p(info), None, 0, _stream()), "cmf_curve_step")
    # a subtraction, a multiply and an add per element and segment; xhat in twice
    _timed("curve_energy", lambda: (3.0 * curves * (points - 1) * n, curves * (8.0 * (points - 1) * n + 8.0 * points + 4.0)), launch)
    return seg2, stats[:, 0], info


def curve_step(T, jtj, cross, xhat, points, damping):
    """One damped Gauss-Newton step per curve: from the Jacobian stack ``T`` of a decode sweep over curves * points
    curve-major samples, its Gram matrices ``jtj`` (curves * points, d, d) float32 (one ``gram_cholesky`` attempt; the lower triangles
    of the interior points are read), ``cross`` of ``cross_gram``, the decoded points ``xhat`` (curves * points, ...) float32 and
    ``damping`` (curves,) float64 >= 0, in float64: the gradient of the interior points and delta = (H + damping diag H)^-1 grad on
    the block tridiagonal Gauss-Newton matrix H.  Returns a ``CurveStepResult``.  Deterministic per curve; one launch, no
    synchronisation."""
    curves, n = _curve_points(xhat, points)
    points, dev = int(points), xhat.device
    _, d = _gram_stack(jtj, "curves * points", "the curve kernels support", GEODESIC_MAX_WIDTH)
    _curve_tangent(T, d, points)
    _check_tensor("cross", cross, torch.float32, f"({curves}, {points - 3}, {d}, {d})", lambda t: t.shape == (curves, points - 3, d, d))
    if T.B != curves * points or T.N != n or jtj.shape[0] != T.B or T.data.device != dev or jtj.device != dev or cross.device != dev:
        raise ValueError(f"T (B = {T.B}, N = {T.N}, nc = {T.nc}) on {T.data.device} must hold d = {d} <= nc columns, nc % 16 == 0, "
                         f"for the {curves * points} samples of {n} elements of xhat on {dev}, like jtj {tuple(jtj.shape)} on "
                         f"{jtj.device} and cross on {cross.device}")
    _check_damping(damping, curves, dev)
    r = CurveStepResult()
    r.grad = torch.empty(curves, points - 2, d, dtype=torch.float64, device=dev)
    r.delta = torch.empty(curves, points - 2, d, dtype=torch.float64, device=dev)
    r.stats = torch.empty(curves, 4, dtype=torch.float64, device=dev)
    r.seg2 = torch.empty(curves, points - 1, dtype=torch.float64, device=dev)
    r.info = torch.empty(curves, dtype=torch.int32, device=dev)
    if curves == 0:
        return r
    lib = _lib.load()
    need = lib.cmf_curve_step_ws(d, points, curves)
    _lib.check(min(need, 0), "cmf_curve_step_ws")
    ws = torch.empty(need, dtype=torch.float64, device=dev)
    launch = lambda: _lib.check(lib.cmf_curve_step(_p(T.data), T.t_b, T.t_r, n, T.nc, d, points, curves, _p(jtj),
                                                   _p(cross) if cross.numel() else None, _p(xhat), _p(damping), _p(r.grad), _p(r.delta),
                                                   _p(r.stats), _p(r.seg2), _p(r.info), _p(ws), need, _stream()), "cmf_curve_step")

    def cost():
        # float64 per curve: J^T s 2 D d per interior point, the block elimination 7 d^3 / 3 per block (d columns on a 2 d window)
        # with the substitutions 6 d^2, the segments 3 D, the forms 5 d^2; bytes: the live quarter-rows of J, three rows of xhat per
        # point, jtj and cross three times, the eliminated columns out and in, the outputs
        M, ncl = points - 2, min(T.nc, -(-d // 4) * 4)
        return (curves * (M * (2.0 * n * d + 7.0 * d ** 3 / 3.0 + 11.0 * d * d) + 3.0 * (points - 1) * n),
                curves * (M * (4.0 * n * ncl + 12.0 * n + 20.0 * d * d + 16.0 * (2 * d + 1) * d + 16.0 * d)
                          + 8.0 * points * n + 8.0 * points + 36.0))
    _timed("curve_step", cost, launch)
    return r


#: most arms of a star ``star_step`` takes (csrc/star_step.hip: the centre kernel reads the arms' codes with one thread each)
STAR_MAX_ARMS = 64


class StarStepResult:
    """Outputs of ``star_step`` (all on the device, float64 unless noted) for stars of K arms of P points, N = P - 1 segments and
    M = P - 2 interior points per arm: ``grad`` (stars, K, M, d) = w_k g_{k,i} and ``grad_centre`` (stars, d) = sum_k w_k g^c_k,
    ``delta`` (stars, K, M, d) and ``delta_centre`` (stars, d), ``seg2`` (stars, K, N) = ||r_i||^2, ``stats`` (stars, 4) =
    [sum_k w_k sum_i ||r_i||^2, g^T delta, delta^T H delta, max |g| over arms and centre], ``info`` (stars,) int32 (0 ok, 1
    non-positive pivot in an arm or at the centre: delta, delta_centre and stats[:, 1:3] NaN, 2 non-finite input: everything NaN)."""
    __slots__ = ("grad", "grad_centre", "delta", "delta_centre", "seg2", "stats", "info")


def star_cross_gram(T, d):
    """The cross-Gram blocks ``star_step`` reads, from the unpadded stack ``T`` of n >= 3 samples: (n - 1, d, d) float32 with block
    q = J_q^T J_{q+1} for q = 1 .. n - 2 and block 0 -- the pair of the first arm's fixed end, which no star reads -- zero.  Two
    ``cmf_cross_gram`` launches on views of the stack as one curve -- all n samples (the pairs 1 .. n - 3), and the last three
    samples with one more behind them that, as a curve's end point, is never read (the pair n - 2) --, so that the decode sweep
    needs no padding samples.  The same arithmetic per pair as ``cross_gram``; no synchronisation."""
    _check_tangent(T)
    _check_on_gpu("T", T.data)
    d, n = int(d), T.B
    _check_width(d, "the curve kernels support", GEODESIC_MAX_WIDTH)
    if n < 3 or T.nc % 16 or T.nc < d or T.nc > GEODESIC_MAX_WIDTH:
        raise ValueError(f"T (B = {n}, nc = {T.nc}) must hold at least 3 samples and d = {d} <= nc <= {GEODESIC_MAX_WIDTH} columns, "
                         f"nc % 16 == 0")
    out = torch.empty(n - 1, d, d, dtype=torch.float32, device=T.data.device)
    out[0].zero_()
    lib = _lib.load()
    at = lambda sample: C.c_void_p(T.data.data_ptr() + 4 * sample * T.t_b)
    block = lambda q: C.c_void_p(out.data_ptr() + 4 * q * d * d)

    def launch():
        if n > 3:
            _lib.check(lib.cmf_cross_gram(at(0), T.t_b, T.t_r, T.N, T.nc, d, n, 1, block(1), _stream()), "cmf_cross_gram")
        _lib.check(lib.cmf_cross_gram(at(n - 3), T.t_b, T.t_r, T.N, T.nc, d, 4, 1, block(n - 2), _stream()), "cmf_cross_gram")
    _timed("cross_gram", lambda: ((n - 2) * 2.0 * T.N * d * d, 4.0 * (n - 2) * (2 * T.N * T.nc + d * d)), launch)
    return out


def star_step(T, jtj, cross, xhat, points, arms, weights, damping, first=0):
    """One damped Gauss-Newton step per star: ``arms`` = K curves of ``points`` points that share a free end point.
    The stack is star-major, then arm-major, point 0 the arm's fixed end and point P - 1 the arm's own copy of the centre:
    ``jtj`` (stars * K * P, d, d) float32 (one ``gram_cholesky`` attempt; lower triangles read), ``cross`` (stars * K * P - 1, d, d)
    float32, block q = J_q^T J_{q+1} of neighbouring samples of the stack (``cross_gram`` on a sweep padded by one sample at each
    end; the blocks that straddle two arms are not read), ``xhat`` (stars * K * P, ...) float32, ``weights`` (stars, K) float64,
    finite and > 0, ``damping`` (stars,) float64 >= 0.  The Jacobian stack ``T`` holds the stack from its sample ``first`` on.  In
    float64: the gradient of sum_k w_k 1/2 sum_i ||r_{k,i}||^2 over the interior points and the centre, and delta = (H + damping
    diag H)^-1 grad on the block-arrow Gauss-Newton matrix, arm by arm with only the centre block shared.  Returns a
    ``StarStepResult``; its sums over arms are taken in arm order.  Deterministic per star; three launches, no synchronisation."""
    points, K, first = int(points), int(arms), int(first)
    if not 1 <= K <= STAR_MAX_ARMS:
        raise ValueError(f"arms = {K}: a star has 1 <= arms <= {STAR_MAX_ARMS}")
    _check_tensor("xhat", xhat, torch.float32, "(stars * arms * points, ...)", lambda t: t.dim() >= 2)
    rows, dev = xhat.shape[0], xhat.device
    stars = _whole_curves(points, rows, "xhat") // K
    n = int(np.prod(xhat.shape[1:]))
    if rows != stars * K * points or n < 1:
        raise ValueError(f"the {rows} samples of xhat {tuple(xhat.shape)} must be whole stars of {K} arms of {points} points with at "
                         f"least one element per point")
    _, d = _gram_stack(jtj, "stars * arms * points", "the star kernels support", GEODESIC_MAX_WIDTH)
    _check_tangent(T)
    _check_on_gpu("T", T.data)
    if T.nc % 16 or T.nc < d or T.nc > GEODESIC_MAX_WIDTH:
        raise ValueError(f"T (nc = {T.nc}) must hold d = {d} <= nc <= {GEODESIC_MAX_WIDTH} columns, nc % 16 == 0")
    _check_tensor("cross", cross, torch.float32, f"({max(rows - 1, 0)}, {d}, {d})", lambda t: t.shape == (max(rows - 1, 0), d, d))
    if first < 0 or T.B < first + rows or T.N != n or jtj.shape[0] != rows or T.data.device != dev or jtj.device != dev or \
            cross.device != dev:
        raise ValueError(f"T (B = {T.B}, N = {T.N}, nc = {T.nc}) on {T.data.device} must hold d = {d} <= nc columns, nc % 16 == 0, "
                         f"for the {rows} samples of {n} elements of xhat on {dev} from its sample {first} on, like jtj "
                         f"{tuple(jtj.shape)} on {jtj.device} and cross on {cross.device}")
    _check_tensor("weights", weights, torch.float64, f"({stars}, {K})", lambda t: t.shape == (stars, K), dev)
    _check_damping(damping, stars, dev)
    M, N = points - 2, points - 1
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
    r = StarStepResult()
    r.grad, r.delta, r.grad_centre, r.delta_centre = f64(stars, K, M, d), f64(stars, K, M, d), f64(stars, d), f64(stars, d)
    r.seg2, r.stats = f64(stars, K, N), f64(stars, 4)
    r.info = torch.empty(stars, dtype=torch.int32, device=dev)
    if stars == 0:
        return r
    lib = _lib.load()
    need = lib.cmf_star_step_ws(d, points, K, stars)
    _lib.check(min(need, 0), "cmf_star_step_ws")
    ws, arm = f64(need), f64(stars, K, 4)
    launch = lambda: _lib.check(lib.cmf_star_step(_p(T.data), T.t_b, T.t_r, n, T.nc, d, points, K, stars, first, _p(jtj), _p(cross),
                                                  _p(xhat), _p(weights), _p(damping), _p(r.grad), _p(r.grad_centre), _p(r.delta),
                                                  _p(r.delta_centre), _p(arm), _p(r.seg2), _p(r.info), _p(ws), need, _stream()),
                                "cmf_star_step")

    def cost():
        # float64 per arm: curve_step's terms with M + 1 streams of J and M full window eliminations; per star the centre's sums
        # 3 K d^2 / 2, its elimination d^3 / 3 and substitutions 2 d^2; bytes: as curve_step per arm, with T_k and r_k out and in
        ncl = min(T.nc, -(-d // 4) * 4)
        return (stars * K * (N * 2.0 * n * d + M * (7.0 * d ** 3 / 3.0 + 11.0 * d * d) + 3.0 * N * n + 1.5 * d * d)
                + stars * (1.5 * K * d * d + d ** 3 / 3.0 + 2.0 * d * d),
                stars * K * (N * (4.0 * n * ncl + 12.0 * n + 12.0 * d * d) + M * (8.0 * d * d + 16.0 * (2 * d + 1) * d + 16.0 * d)
                             + 8.0 * points * n + 8.0 * points + 8.0 * d * d + 32.0 * d + 40.0) + stars * (16.0 * d + 4.0))
    _timed("star_step", cost, launch)
    # the star's figures from the arms', summed in arm order
    total = [torch.zeros(stars, dtype=torch.float64, device=dev) for _ in range(3)]
    for k in range(K):
        for j in range(3):
            total[j] = total[j] + weights[:, k] * arm[:, k, j]
    gmax = torch.maximum((weights * arm[:, :, 3]).amax(1), r.grad_centre.abs().amax(1))
    r.stats = torch.stack(total + [gmax], 1)
    return r


#: widest metric ``tangent_pca`` takes: the float64 matrix of a group lives in LDS (csrc/tangent_pca.hip)
TANGENT_PCA_MAX_WIDTH = 128


class TangentPcaResult:
    """Outputs of ``tangent_pca`` (all on the device, float64 unless noted) for groups of K tangent vectors and r components:
    ``variances`` (B, r) descending, ``directions`` (B, r, d) = u_j, ``scores`` (B, K, r) = u_j^T G v_k, ``covectors`` (B, K, d) =
    G v_k, ``norm2`` (B, K) = v_k^T G v_k, ``total`` (B,) = sum_k w_k norm2_k / sum_k w_k, ``rank`` and ``sweeps`` (B,) int32,
    ``info`` (B,) int32 (0 ok, 1 sweep cap reached, 2 a non-finite input or a weight that is not finite and > 0: every float output
    of the group NaN, rank 0)."""
    __slots__ = ("variances", "directions", "scores", "covectors", "norm2", "total", "rank", "sweeps", "info")


def tangent_pca(jtj, vectors, weights, components=None):
    """Principal geodesic analysis per group: PCA of the K tangent vectors ``vectors`` (B, K, d) float64 with the
    ``weights`` (B, K) float64, finite and > 0, in the metric ``jtj`` (B, d, d) float32 (one ``gram_cholesky`` attempt; lower
    triangles read), in its dual K x K form by the float64 Jacobi method of ``gram_spectrum``, one workgroup per group.
    ``components`` = r, 1 <= r <= K (default K), modes are returned; those beyond the numerical rank -- eigenvalues not above
    d 2^-24 times the largest, which a float32 metric leaves undetermined -- have zero directions and scores.  Returns a
    ``TangentPcaResult``.  Deterministic per group; enqueues one launch, no synchronisation."""
    B, d = _gram_stack(jtj, "B", "the tangent PCA kernel supports", TANGENT_PCA_MAX_WIDTH)
    dev = jtj.device
    _check_tensor("vectors", vectors, torch.float64, f"({B}, K, {d})", lambda t: t.dim() == 3 and t.shape[0] == B and t.shape[2] == d,
                  dev)
    K = vectors.shape[1]
    if not 1 <= K <= STAR_MAX_ARMS:
        raise ValueError(f"vectors {tuple(vectors.shape)}: a group has 1 <= K <= {STAR_MAX_ARMS} tangent vectors")
    _check_tensor("weights", weights, torch.float64, f"({B}, {K})", lambda t: t.shape == (B, K), dev)
    r_ = K if components is None else int(components)
    if not 1 <= r_ <= K:
        raise ValueError(f"components = {components}: need 1 <= components <= K = {K}")
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    r = TangentPcaResult()
    r.variances, r.directions, r.scores, r.covectors = f64(B, r_), f64(B, r_, d), f64(B, K, r_), f64(B, K, d)
    r.norm2, r.total = f64(B, K), f64(B)
    r.rank, r.sweeps, r.info = i32(B), i32(B), i32(B)
    if B == 0:
        return r
    launch = lambda: _lib.check(_lib.load().cmf_tangent_pca(_p(jtj), _p(vectors), _p(weights), d, K, r_, B, _p(r.variances),
                                                            _p(r.directions), _p(r.scores), _p(r.covectors), _p(r.norm2),
                                                            _p(r.total), _p(r.rank), _p(r.sweeps), _p(r.info), _stream()),
                                "cmf_tangent_pca")
    # float64: G v_k 2 K d^2, the K (K + 1) / 2 dots of length d, a nominal 10 sweeps of K (K - 1) / 2 rotations of 6 FLOP on 3 K
    # entry pairs (M twice, P once), the r directions 3 K d each; bytes: jtj, vectors (three times), weights in, the outputs out
    # and covectors, directions in again
    _timed("tangent_pca", lambda: (B * (2.0 * K * d * d + K * (K + 1.0) * d + 10.0 * (K * (K - 1) / 2) * 18.0 * K + 3.0 * r_ * K * d),
                                   B * (4.0 * d * d + 24.0 * K * d + 8.0 * K + 16.0 * K * d + 8.0 * r_ + 24.0 * r_ * d
                                        + 8.0 * K * r_ + 8.0 * K + 20.0)), launch)
    return r


#: widest metric ``metric_solve`` takes: the float64 matrix of a sample lives in LDS (csrc/shoot_step.hip)
SHOOT_MAX_WIDTH = 128


class MetricSolveResult:
    """Outputs of ``metric_solve`` (all on the device): ``out64`` (B, d) float64 = G^-1 rhs (or G rhs), ``out32`` (B, d) float32,
    the same values rounded, ``stats`` (B, 2) float64 = [rhs^T out, max |out_k|], ``info`` (B,) int32 (0 ok, 1 non-positive pivot:
    out and stats NaN, 2 non-finite input: everything NaN)."""
    __slots__ = ("out64", "out32", "stats", "info")


def metric_solve(jtj, rhs, apply=False):
    """The per-sample float64 step of geodesic shooting: from the Gram matrix ``jtj`` (B, d, d) float32 (one
    ``gram_cholesky`` attempt; the lower triangles are read) and ``rhs`` (B, d) float64, out = G^-1 rhs -- the velocity of a
    momentum, ``stats[:, 0]`` the squared speed -- or, with ``apply``, out = G rhs -- the momentum of a velocity.  Returns a
    ``MetricSolveResult``; ``out32[:, :, None]`` is the ``eps`` of a one-direction sweep.  Deterministic per sample; one launch,
    no synchronisation."""
    B, d = _gram_stack(jtj, "B", "the metric solve kernel supports", SHOOT_MAX_WIDTH)
    dev = jtj.device
    _check_tensor("rhs", rhs, torch.float64, f"({B}, {d})", lambda t: t.shape == (B, d), dev)
    r = MetricSolveResult()
    r.out64 = torch.empty(B, d, dtype=torch.float64, device=dev)
    r.out32 = torch.empty(B, d, dtype=torch.float32, device=dev)
    r.stats = torch.empty(B, 2, dtype=torch.float64, device=dev)
    r.info = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return r
    launch = lambda: _lib.check(_lib.load().cmf_metric_solve(_p(jtj), _p(rhs), d, B, int(bool(apply)), _p(r.out64), _p(r.out32),
                                                             _p(r.stats), _p(r.info), _stream()), "cmf_metric_solve")
    # float64: the elimination d^3 / 3 with the two substitutions 2 d^2 (apply: the product 2 d^2), the form 2 d; bytes: the
    # triangle of G and rhs in, the outputs
    _timed("metric_solve", lambda: (B * ((2.0 * d * d if apply else d ** 3 / 3.0 + 2.0 * d * d) + 2.0 * d),
                                    B * (2.0 * d * (d + 1) + 20.0 * d + 20.0)), launch)
    return r


#: widest metric ``transport_chain`` takes, and the vectors of one launch (one column group): the float64 window of a curve --
#: a matrix and its right-hand sides -- lives in LDS (csrc/transport_step.hip)
TRANSPORT_MAX_WIDTH = 128
TRANSPORT_MAX_VECTORS = 16


class TransportResult:
    """Outputs of ``transport_chain`` (all on the device, float64 unless noted) for curves of P points and N = P - 1 segments with m
    vectors each: ``out`` (curves, P, m, d), the vectors at every point (``out[:, 0]`` = w0); ``fwd`` and ``bwd`` (curves, N, m, d),
    the two halves of every segment, ``out[:, i + 1]`` = (fwd[:, i] + bwd[:, i]) / 2; ``norm2`` (curves, P, m) = w^T G w; ``info``
    (curves,) int32 (0 ok; 1 a failed pivot in segment i: fwd / bwd from segment i on and out / norm2 from point i + 1 on NaN; 2
    non-finite input: everything NaN)."""
    __slots__ = ("out", "fwd", "bwd", "norm2", "info")


def transport_chain(jtj, cross, w0, points):
    """Parallel transport along curve-major curves of ``points`` points: from the Gram matrices ``jtj``
    (curves * points, d, d) float32 (one ``gram_cholesky`` attempt; the lower triangles are read), the cross-Gram blocks ``cross``
    (curves * points - 1, d, d) float32 of neighbouring samples of the stack (block s = J_s^T J_{s+1}; those that straddle two curves
    are not read) and the vectors ``w0`` (curves, m, d) float64 at the first points, in float64 per segment: fwd = G_{i+1}^-1 C_i^T w,
    bwd = C_i^-1 G_i w, w <- (fwd + bwd) / 2.  Returns a ``TransportResult``.  Deterministic per curve; one launch, no
    synchronisation."""
    rows, d = _gram_stack(jtj, "curves * points", "the transport kernel supports", TRANSPORT_MAX_WIDTH)
    dev, points = jtj.device, int(points)
    curves = _whole_curves(points, rows, "jtj", least=2)
    _check_tensor("w0", w0, torch.float64, f"({curves}, m, {d})", lambda t: t.dim() == 3 and t.shape[0] == curves and t.shape[2] == d, dev)
    m = w0.shape[1]
    if not 1 <= m <= TRANSPORT_MAX_VECTORS:
        raise ValueError(f"m = {m}: the transport kernel takes 1 <= m <= {TRANSPORT_MAX_VECTORS} vectors per launch")
    _check_tensor("cross", cross, torch.float32, f"({max(rows - 1, 0)}, {d}, {d})", lambda t: t.shape == (max(rows - 1, 0), d, d), dev)
    r = TransportResult()
    r.out = torch.empty(curves, points, m, d, dtype=torch.float64, device=dev)
    r.fwd = torch.empty(curves, points - 1, m, d, dtype=torch.float64, device=dev)
    r.bwd = torch.empty(curves, points - 1, m, d, dtype=torch.float64, device=dev)
    r.norm2 = torch.empty(curves, points, m, dtype=torch.float64, device=dev)
    r.info = torch.empty(curves, dtype=torch.int32, device=dev)
    if curves == 0:
        return r
    launch = lambda: _lib.check(_lib.load().cmf_transport_chain(_p(jtj), _p(cross), _p(w0), d, m, points, curves, _p(r.out), _p(r.fwd),
                                                                _p(r.bwd), _p(r.norm2), _p(r.info), _stream()), "cmf_transport_chain")

    def cost():
        # float64 per segment: the LU 2 d^3 / 3 and the Cholesky d^3 / 3 with their right-hand sides 3 m d^2 and the substitutions
        # 3 m d^2, the two products 4 m d^2; bytes: jtj three times (the check, the product, the triangle), cross three times, the outputs
        N = points - 1
        return (curves * (N * (d ** 3 + 10.0 * m * d * d) + 2.0 * points * m * d * d),
                curves * (12.0 * (points + N) * d * d + 8.0 * (points + 2 * N) * m * d + 8.0 * m * d + 8.0 * points * m + 4.0))
    _timed("transport_chain", cost, launch)
    return r


#: widest Jacobian ``second_form`` takes, and the directions of one frame: the float64 window of a sample -- the metric and the
#: m (m + 1) / 2 right-hand sides -- lives in LDS (csrc/second_form.hip)
CURVATURE_MAX_WIDTH = 128
CURVATURE_MAX_FRAME = 4


class SecondFormResult:
    """Outputs of ``second_form`` (all on the device, float64 unless noted) for B samples, frames of m directions and q = m (m + 1) / 2
    pairs (a, b), a <= b, a-major: ``second_gram`` (B, q, q), the Gram matrix of the normal components II_ab, whole; ``christoffel``
    (B, q, d) = G^-1 J^T H_ab; ``frame_metric`` (B, m, m) = u_a^T G u_b; ``stats`` (B, 4) = [sum_{a<b} ||D_ab - D_ba||^2,
    sum_{a<b} ||H_ab||^2, trace H^T H, trace second_gram]; ``info`` (B,) int32 (0 ok; 1 non-positive pivot of G: second_gram,
    christoffel, stats[:, 3] NaN; 2 non-finite input or a step that is not finite and > 0: everything NaN)."""
    __slots__ = ("second_gram", "christoffel", "frame_metric", "stats", "info")


def second_form(T, jtj, S, frame, step):
    """The per-sample float64 reduction of the curvature estimate: from the Jacobian stack ``T`` of a decode sweep at B
    latents, its Gram matrix ``jtj`` (B, d, d) float32 (one ``gram_cholesky`` attempt; the lower triangles are read), ``frame``
    (B, m, d) float64 -- m <= min(d, 4) unit latent directions per sample --, ``step`` (B,) float64 > 0 and the 16-column sweep ``S``
    over the 2 m B shifted latents (sample (b m + a) 2 + sign at z_b +- step_b frame[b, a], column c < m = J frame[b, c]): the
    symmetrised central differences H_ab, the Gram matrix of their normal components (a Schur complement), the Christoffel
    contractions G^-1 J^T H_ab and the metric of the frame.  Returns a ``SecondFormResult``.  Deterministic per sample; one launch, no
    synchronisation."""
    _check_tangent(T)
    if not isinstance(S, Tangent):
        raise ValueError(f"S must be an engine.Tangent, got {type(S).__name__}")
    B, d = _gram_stack(jtj, "B", "the second-form kernel supports", CURVATURE_MAX_WIDTH)
    dev = jtj.device
    _check_tensor("frame", frame, torch.float64, f"({B}, m, {d})", lambda t: t.dim() == 3 and t.shape[0] == B and t.shape[2] == d, dev)
    m = frame.shape[1]
    if not 1 <= m <= min(d, CURVATURE_MAX_FRAME):
        raise ValueError(f"m = {m}: the second-form kernel takes frames of 1 <= m <= min(d, {CURVATURE_MAX_FRAME}) = "
                         f"{min(d, CURVATURE_MAX_FRAME)} directions")
    _check_tensor("step", step, torch.float64, f"({B},)", lambda t: t.shape == (B,), dev)
    if T.B != B or T.nc % 16 or T.nc < d or T.N < 1 or T.data.device != dev:
        raise ValueError(f"T (B = {T.B}, N = {T.N}, nc = {T.nc}) on {T.data.device} must hold d = {d} <= nc columns, nc % 16 == 0, for "
                         f"the {B} samples of jtj on {dev}")
    if S.B != 2 * m * B or S.N != T.N or S.nc != 16 or S.nc < m or S.data.device != dev:
        raise ValueError(f"S (B = {S.B}, N = {S.N}, nc = {S.nc}) on {S.data.device} must hold the 2 m B = {2 * m * B} shifted samples "
                         f"of {T.N} elements in 16 >= m = {m} columns on {dev}")
    q = m * (m + 1) // 2
    r = SecondFormResult()
    r.second_gram = torch.empty(B, q, q, dtype=torch.float64, device=dev)
    r.christoffel = torch.empty(B, q, d, dtype=torch.float64, device=dev)
    r.frame_metric = torch.empty(B, m, m, dtype=torch.float64, device=dev)
    r.stats = torch.empty(B, 4, dtype=torch.float64, device=dev)
    r.info = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return r
    n = T.N
    launch = lambda: _lib.check(_lib.load().cmf_second_form(_p(T.data), T.t_b, T.t_r, n, T.nc, d, m, B, _p(jtj), _p(S.data), S.t_b,
                                                            S.t_r, _p(frame), _p(step), _p(r.second_gram), _p(r.christoffel),
                                                            _p(r.frame_metric), _p(r.stats), _p(r.info), _stream()), "cmf_second_form")

    def cost():
        # float64: the differences 3 m^2 D, J^T H 2 D d q, H^T H and the two asymmetry sums 2 D (q (q + 1) / 2 + m (m - 1)), the
        # elimination d^3 / 3 with its q rows q d^2, the Schur complement 3 d q (q + 1) / 2, the back substitution q d^2, the frame's
        # metric 2 m d^2; bytes: the live quarter-rows of J, the first quarter-rows of S twice (L2 the second time), the triangle of G,
        # the frame, the outputs
        ncl = min(T.nc, -(-d // 4) * 4)
        return (B * (3.0 * m * m * n + 2.0 * n * d * q + 2.0 * n * (q * (q + 1) / 2 + m * (m - 1)) + d ** 3 / 3.0 + 2.0 * q * d * d
                     + 1.5 * d * q * (q + 1) + 2.0 * m * d * d),
                B * (4.0 * n * ncl + 2 * 16.0 * n * 2 * m + 2.0 * d * (d + 1) + 8.0 * m * d + 8.0 * (q * q + q * d + m * m + 5) + 4.0))
    _timed("second_form", cost, launch)
    return r


def gram_backward(T, jtj, g_logdet=None, g_l1off=None, g_l1diag=None):
    """Cotangent of the Jacobian stack T for a loss with d/d logdet = g_logdet, d/d l1_off = g_l1off, d/d l1_diag =
    g_l1diag (each (B,) or None): what autograd yields through non_square.py:307-308, :280-294, :87-100."""
    B, d = jtj.shape[0], jtj.shape[1]
    assert B == T.B and d <= T.nc
    check_latent_width(d)
    dT = T.like(T.N)
    gs = [None if g is None else g.to(torch.float32).contiguous() for g in (g_logdet, g_l1off, g_l1diag)]
    if T.nc > WIDE_NC:
        # G^-1 from a Cholesky factorisation in a workspace (factor + the d x d cotangent): torch-allocated, so a captured
        # graph's pool serves it
        ws = torch.empty(2 * B * d * d, dtype=torch.float32, device=T.data.device)
        launch = lambda: _lib.check(_lib.load().cmf_gram_backward_ws(
            _p(T.data), T.t_b, T.t_r, T.N, T.nc, d, B, _p(jtj), *[None if g is None else _p(g) for g in gs], _p(dT.data), dT.t_b,
            dT.t_r, _p(ws), _stream()), "cmf_gram_backward_ws")
        # factor d^3/3, inverse ~d^3, product 2 D NC d; panel in and out, 4 d^2 of ws
        _timed("gram_backward_wide", lambda: (B * (d ** 3 * 4 / 3.0 + 2.0 * T.N * T.nc * d), 4.0 * B * (2 * T.N * T.nc + 6 * d * d)),
               launch)
        return dT
    _lib.check(_lib.load().cmf_gram_backward(_p(T.data), T.t_b, T.t_r, T.N, T.nc, d, B, _p(jtj),
                                             *[None if g is None else _p(g) for g in gs], _p(dT.data), dT.t_b, dT.t_r,
                                             _stream()), "cmf_gram_backward")
    return dT


def gram_backward_matrix(T, M):
    """dT = T (M + M^T) for an explicit cotangent M (B, d, d) of the Gram matrix (Hutchinson surrogate training)."""
    B, d = M.shape[0], M.shape[1]
    assert B == T.B and d <= T.nc
    check_latent_width(d)
    dT = T.like(T.N)
    Mc = M.to(torch.float32).contiguous()
    launch = lambda: _lib.check(_lib.load().cmf_gram_backward_matrix(_p(T.data), T.t_b, T.t_r, T.N, T.nc, d, B, _p(Mc), _p(dT.data),
                                                                     dT.t_b, dT.t_r, _stream()), "cmf_gram_backward_matrix")
    _timed("gram_backward_matrix_wide" if T.nc > WIDE_NC else None,
           lambda: (2.0 * B * T.N * T.nc * d, 4.0 * B * (2 * T.N * T.nc + 2 * d * d)), launch)
    return dT


def hutch_cg(jtj, eps, max_iter, tol, min_iter=None):
    """Hutchinson surrogate on explicit J^T J: returns (value (B,), u, w (B,d,S), iterations (B,))."""
    B, d, S = eps.shape
    check_latent_width(d)
    if min_iter is None:
        min_iter = min(10, max_iter - 1) + 1 if max_iter > 1 else 1
    dev = eps.device
    u, w = torch.empty_like(eps), torch.empty_like(eps)
    val = torch.empty(B, dtype=torch.float32, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    ec = eps.contiguous()
    launch = lambda: _lib.check(_lib.load().cmf_hutch_cg(_p(jtj), _p(ec), d, S, B, int(max_iter), int(min_iter), float(tol), _p(u),
                                                         _p(w), _p(val), _p(iters), _stream()), "cmf_hutch_cg")
    # per iteration (at most max_iter) one G read per 16-probe chunk
    _timed("hutch_cg_wide" if d > WIDE_NC or S > WIDE_NC else None,
           lambda: (2.0 * B * d * d * S * (max_iter + 1), 4.0 * B * d * d * -(-S // 16) * (max_iter + 1)), launch)
    return val, u, w, iters


def hutch_metric(w):
    """(l1_off, l1_diag) of the Hutchinson product W = (J^T J) eps, (B, d, S) (non_square.py:87-100 on :253-258).  The
    off-diagonal sum exists only for S == d (the reference's ``view`` at :98; None otherwise); the diagonal one is
    ``torch.diagonal`` of the rectangular block: min(d, S) entries (:87-92)."""
    B, d, S = w.shape
    check_latent_width(d)
    off = torch.empty(B, dtype=torch.float32, device=w.device) if S == d else None
    diag = torch.empty(B, dtype=torch.float32, device=w.device)
    _lib.check(_lib.load().cmf_hutch_metric(_p(w.contiguous()), d, S, B, _p(off), _p(diag), _stream()), "cmf_hutch_metric")
    return off, diag


def hutch_cotangent(u, eps, w, g_val=None, g_off=None, g_diag=None):
    """d objective / d (J^T J) as an explicit (B, d, d) matrix for the train-mode Hutchinson objective (u detached)."""
    B, d, S = eps.shape
    check_latent_width(d)
    M = torch.empty(B, d, d, dtype=torch.float32, device=eps.device)
    gs = [None if g is None else g.to(torch.float32).contiguous() for g in (g_val, g_off, g_diag)]
    uc, ec, wc = u.contiguous(), eps.contiguous(), w.contiguous()
    launch = lambda: _lib.check(_lib.load().cmf_hutch_cotangent(_p(uc), _p(ec), _p(wc), d, S, B, *[None if g is None else _p(g) for g in gs],
                                                                _p(M), _stream()), "cmf_hutch_cotangent")
    _timed("hutch_cotangent_wide" if d > WIDE_NC or S > WIDE_NC else None,
           lambda: (2.0 * B * d * d * S, 4.0 * B * (3 * d * S + d * d)), launch)
    return M


def hutch_lowrank_cotangent(w, S, g_val=None, g_diag=None):
    """(B, n, n) cotangent of P^T P for the n-column sweep P = J [u | eps | e_0..e_{K-1}] of the low-rank Hutchinson backward
    (``cmf_hutch_lowrank_cotangent``); n = 2 S + (min(d, S) if g_diag is given)."""
    B, d = w.shape[0], w.shape[1]
    check_latent_width(d)
    n = 2 * S + (min(d, S) if g_diag is not None else 0)
    M = torch.empty(B, n, n, dtype=torch.float32, device=w.device)
    gs = [None if g is None else g.to(torch.float32).contiguous() for g in (g_val, g_diag)]
    _lib.check(_lib.load().cmf_hutch_lowrank_cotangent(_p(w.contiguous()), d, S, B, *[None if g is None else _p(g) for g in gs], n,
                                                       _p(M), _stream()), "cmf_hutch_lowrank_cotangent")
    return M


# --------------------------------------------------------------------------------------------------
# NSF prior layers: derived weights are cached per parameter version like the packs
# --------------------------------------------------------------------------------------------------


class _DerivedCache:
    """Tensors computed from parameters by a kernel (masked MADE weights, L U products), rebuilt when a source parameter
    changes (``_version`` / storage / ``PACKS.generation``, which FlatOptimizer bumps).  A stale entry is rebuilt INTO its old
    tensors (same identity, ``_version`` bumped by the copy), so the pack cache entry keyed on that identity is refreshed in place
    instead of a new one piling up per optimiser step."""

    def __init__(self):
        self._store = {}

    def get(self, key, sources, build):
        import weakref
        ver = tuple((s._version, s.data_ptr(), s.device) for s in sources) + (PACKS.generation,)
        hit = self._store.get(key)
        if hit is not None and hit[0]() is sources[0] and hit[1] == ver:
            return hit[2]
        out = build()
        if hit is not None and hit[0]() is sources[0]:
            # same layout as the stale entry (equal shapes / dtypes; equal non-tensor parts such as offsets and widths): refresh
            # the OLD tensors in place, so whatever is keyed on their identity (the pack cache) follows instead of piling up
            olds, news = (hit[2], out) if isinstance(out, tuple) else ((hit[2],), (out,))
            same = len(olds) == len(news) and all(
                (o.shape == n.shape and o.dtype == n.dtype and o.device == n.device) if torch.is_tensor(o) and torch.is_tensor(n)
                else (not torch.is_tensor(o) and not torch.is_tensor(n) and o == n) for o, n in zip(olds, news))
            if same:
                for o, n in zip(olds, news):
                    if torch.is_tensor(o):
                        o.copy_(n)
                out = hit[2]
        if len(self._store) > 4096:
            self._store = {k: v for k, v in self._store.items() if v[0]() is not None}
        self._store[key] = (weakref.ref(sources[0]), ver, out)
        return out


DERIVED = _DerivedCache()


#: fused coupling layers for MLP couplers (cmf_mlp_coupler): False = always the per-layer launches (the training path
#: always uses them: it needs every layer's state)
FUSED_MLP = True


def mlp_coupler_supported(net, view, T, n_out):
    """Shapes the fused kernel covers: tanh MLP, <= 8 linear layers, hidden <= 128, outputs <= 64, inputs <= 128; with
    tangents: 16 column slots of which at most 15 are Jacobian columns (column 15 carries the primal)."""
    if not FUSED_MLP or net.kind != "mlp" or view.mask is not None:
        return False
    lins = [m for m in net if isinstance(m, nn.Linear)]
    if not 2 <= len(lins) <= _lib.MLP_MAX_LAYERS or view.cin > 128 or n_out > 64:
        return False
    if any(l.out_features > 128 for l in lins[:-1]):
        return False
    return T is None or (T.layout == "fmajor" and T.nc == 16)


def _mlp_images(net):
    """All layer images of an MLP coupler net back to back (cmf_pack_mlp_layer), cached per parameter version:
    (flat tensor, float offsets, widths)."""
    lins = [m for m in net if isinstance(m, nn.Linear)]
    params = [p for l in lins for p in (l.weight, l.bias)]

    def build():
        lib = _lib.load()
        ht = lib.cmf_mlp_hidden_tiles(max(l.out_features for l in lins[:-1]))
        tiles = [(ht if i + 1 < len(lins) else (l.out_features + 15) // 16, ht if i > 0 else (l.in_features + 15) // 16)
                 for i, l in enumerate(lins)]                    # (output tiles, input K groups) per layer
        sizes = []
        for l, (mt, kg) in zip(lins, tiles):
            n = C.c_longlong(0)
            _lib.check(lib.cmf_pack_mlp_layer(None, None, l.out_features, l.in_features, 0, mt, kg, None, C.byref(n), None), "pack size")
            sizes.append((n.value + 3) // 4 * 4)
        offs = [0]
        for n in sizes[:-1]:
            offs.append(offs[-1] + n)
        flat = torch.zeros(sum(sizes), dtype=torch.float32, device=lins[0].weight.device)
        for i, (l, (mt, kg)) in enumerate(zip(lins, tiles)):
            _lib.check(lib.cmf_pack_mlp_layer(_p(l.weight.detach().contiguous()), _p(l.bias.detach().contiguous()), l.out_features,
                                              l.in_features, int(i == 0), mt, kg, C.c_void_p(flat.data_ptr() + 4 * offs[i]), None,
                                              _stream()), "cmf_pack_mlp_layer")
        return flat, offs, [lins[0].in_features] + [l.out_features for l in lins]

    return DERIVED.get((id(lins[0].weight), "mlp-images"), params, build)


def mlp_coupler(net, z, T, view, maps, decode, lj=None, ncols=None):
    """One fused coupling layer with an MLP coupler: in place on ``z`` (B, D) and, with a tangent stack ``T`` (fmajor, 16
    columns of which ``ncols`` <= 15 are used), on the modified rows of ``T``."""
    flat, offs, widths = _mlp_images(net)
    B = z.shape[0]
    z2 = z.view(B, -1)
    a = _lib.MlpCouplerArgs()
    a.z, a.z_b = _p(z2), z2.shape[1]
    if T is not None:
        assert decode and T.layout == "fmajor" and T.nc == 16 and (ncols is None or ncols <= 15)
        a.t, a.t_f = _p(T.data), T.t_r
    a.w = _p(flat)
    a.zi, a.si, a.ti, a.n_mod = _p(maps["zi"]), _p(maps["si"]), _p(maps["ti"]), maps["n"]
    a.B, a.cin, a.chan_off, a.chan_step = B, view.cin, view.chan_off, view.chan_step
    a.n_layers = len(offs)
    for i, w_ in enumerate(widths):
        a.width[i] = w_
    for i, o in enumerate(offs):
        a.w_off[i] = o
    a.decode = int(decode)
    a.lj = _p(lj)
    a.ncols = int(ncols) if (T is not None and ncols is not None) else 15
    launch = lambda: _lib.check(_lib.load().cmf_mlp_coupler(C.byref(a), _stream()), "cmf_mlp_coupler")

    def cost():
        # algorithmic work: 2 in out FLOP per layer and column (1 primal + ncols tangents, or 1 per sample in primal mode)
        cols = (1 + (ncols if ncols is not None else 15)) if T is not None else 1
        fl = 2.0 * B * cols * sum(widths[i] * widths[i + 1] for i in range(len(widths) - 1))
        by = 4.0 * B * cols * (view.cin + 2 * maps["n"])
        return fl, by
    return _timed("mlp_coupler" + ("_tangent" if T is not None else "_primal"), cost, launch)


def made_masked_weight(weight, kind, features, multiplier=1):
    """weight * MADE mask (kind 0 input->hidden, 1 hidden->hidden, 2 hidden->output) as a cached (out, in) tensor."""
    def build():
        w = weight.detach().contiguous()
        out = torch.empty_like(w)
        _lib.check(_lib.load().cmf_made_mask_weight(_p(w), _p(out), w.shape[0], w.shape[1], int(kind), int(features),
                                                    int(multiplier), _stream()), "cmf_made_mask_weight")
        return out
    return DERIVED.get((id(weight), "made", kind, features, multiplier), [weight], build)


def lu_weights(lower, upper, udiag, eps=1e-3):
    """(W = L U (n, n), logabsdet (1,)) of an LULinear layer, cached per parameter version."""
    def build():
        n = udiag.shape[0]
        W = torch.empty(n, n, dtype=torch.float32, device=udiag.device)
        ld = torch.empty(1, dtype=torch.float32, device=udiag.device)
        _lib.check(_lib.load().cmf_lu_weights(_p(lower.detach().contiguous()), _p(upper.detach().contiguous()),
                                              _p(udiag.detach().contiguous()), n, float(eps), _p(W), _p(ld), _stream()),
                   "cmf_lu_weights")
        return W, ld
    return DERIVED.get((id(udiag), "lu"), [udiag, lower, upper], build)


def linear_primal(x, weight, bias, relu_in=False, res=None):
    """y (B, out) = W [relu](x) + b [+ res] through ``cmf_conv_primal`` with taps = 1 (pixels = samples)."""
    B, cin = x.shape
    cout = weight.shape[0]
    y = torch.empty(B, cout, dtype=torch.float32, device=x.device)
    conv_primal(x, 0, 0, 1, cin, weight, 1, bias, y, 0, 1, cout, 1, cin, cout, 1, B, imode=F_RELU if relu_in else F_NONE, res=res)
    return y


class GroupedBatch:
    """(B, F) tensors with 16 samples in the 16 column slots of the tangent-conv kernels -- (G, F, 16), viewed as ONE image row of
    G pixels -- for the backward of small linear layers (MLP couplers, the nsf prior's MADE and LULinear) on those kernels; or (B, C, H,
    W) tensors as (G, C, HW, 16) images (ResNet couplers).  Zero-padded to a multiple of ``multiple`` samples (CouplerPlan.multiple)."""

    def __init__(self, B, device, multiple=16):
        self.B, self.Bp, self.dev = B, (B + multiple - 1) // multiple * multiple, device
        self.G = self.Bp // 16

    def pack(self, t):
        t = t.reshape(self.B, -1)
        if self.Bp != self.B:
            t = torch.cat([t, torch.zeros(self.Bp - self.B, t.shape[1], dtype=t.dtype, device=self.dev)])
        return primal_regroup(t.contiguous(), True)

    def unpack(self, t_g, F):
        return primal_regroup(t_g.view(self.G, -1), False).view(self.Bp, F)[: self.B]

    @staticmethod
    def strides(c):
        return (0, 16, c * 16)                               # (np, chan, px)

    @staticmethod
    def image_strides(c, HW):
        return (c * HW * 16, HW * 16, 16)                    # (np, chan, px) of a grouped image tensor (G, c, HW, 16)

    def linear_backward(self, x_g, dy_g, weight, cin, cout, dw=None, db=None, relu_in=False, fo_g=None, res_g=None):
        """y = W [relu](x) + b on grouped tensors: dw += sum dy (x) [relu](x), db += sum dy, returns W^T dy (optionally
        times [fo > 0], plus res)."""
        if dw is not None:
            conv_tangent_wgrad(x_g, 0, *self.strides(cin), dy_g, 0, *self.strides(cout), dw, 1, 1, cin, cout, 1, self.G, 16,
                               fmode=F_SELF_RELU if relu_in else F_NONE)
        if db is not None:
            channel_sum(dy_g, *self.strides(cout), 1, cout, self.G, 16, db)
        dx_g = torch.empty(self.G * cin * 16, dtype=torch.float32, device=self.dev)
        fo = {} if fo_g is None else dict(fo=fo_g, fo_np=0, fo_co=16, fo_px=cin * 16, fomode=F_SELF_RELU)
        conv_tangent(dy_g, 0, *self.strides(cout), weight, 1, dx_g, *self.strides(cin), 1, cout, cin, 1, self.G, 16,
                     transpose=True, precision="f32", res_t=res_g, **fo)
        return dx_g


def rq_spline_backward(x, params, bins, hidden, tail_bound, dz, dlj=None):
    """(dx (B, D), dparams (B, D * (3 bins - 1))) of the forward spline for the cotangents dz (B, D) and dlj (B,)."""
    B, D = x.shape
    dx = torch.empty_like(x)
    dparams = torch.empty_like(params)
    _lib.check(_lib.load().cmf_rq_spline_backward(_p(x), D, _p(params), D, int(bins), int(hidden), float(tail_bound), B,
                                                  _p(dz.contiguous()), D, _p(dlj), _p(dx), D, _p(dparams), _stream()),
               "cmf_rq_spline_backward")
    return dx, dparams


def rq_spline(x, params, bins, hidden, tail_bound, inverse=False, lj=None):
    """Elementwise rational-quadratic spline with linear tails on (B, D); params (B, D * (3 bins - 1)); lj (B,) accumulates."""
    B, D = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().cmf_rq_spline(_p(x), D, _p(params), D, int(bins), int(hidden), float(tail_bound), int(inverse), B,
                                         _p(out), D, _p(lj), _stream()), "cmf_rq_spline")
    return out


def prehead(x, noise, a, c, logit):
    B = x.shape[0]
    n = x[0].numel()
    y = torch.empty_like(x)
    lj = torch.empty(B, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().cmf_prehead(_p(x), _p(noise), _p(y), _p(lj), float(a), float(c), int(logit), n, B, _stream()),
               "cmf_prehead")
    return y, lj


def prehead_inverse(y, a, c, logit):
    x = torch.empty_like(y)
    _lib.check(_lib.load().cmf_prehead_inverse(_p(y), _p(x), float(a), float(c), int(logit), y.numel(), _stream()),
               "cmf_prehead_inverse")
    return x


def gaussian_logprob(z, lp):
    B = z.shape[0]
    z2 = z.view(B, -1)
    _lib.check(_lib.load().cmf_gaussian_logprob(_p(z2), z2.shape[1], z2.shape[1], B, _p(lp), _stream()),
               "cmf_gaussian_logprob")


def affine_prior(z, log_scale, shift, decode, lj=None):
    B = z.shape[0]
    z2 = z.view(B, -1)
    _lib.check(_lib.load().cmf_affine_prior(_p(z2), z2.shape[1], _p(log_scale.detach().contiguous()),
                                            _p(shift.detach().contiguous()), z2.shape[1], B, int(decode), _p(lj), _stream()),
               "cmf_affine_prior")


def recon_sqerr(xh, x):
    B = x.shape[0]
    rec = torch.empty(B, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().cmf_recon_sqerr(_p(xh.reshape(B, -1)), _p(x.reshape(B, -1)), x[0].numel(), B, _p(rec), _stream()),
               "cmf_recon_sqerr")
    return rec


def elbo_combine(low, logdet, rec, l1, pre, wl, lam, wm, B, device):
    out = torch.empty(B, 1, dtype=torch.float32, device=device)
    _lib.check(_lib.load().cmf_elbo_combine(_p(low), _p(logdet), _p(rec), _p(l1), _p(pre), float(wl), float(lam), float(wm),
                                            B, _p(out), _stream()), "cmf_elbo_combine")
    return out


# --------------------------------------------------------------------------------------------------
# coupler networks
# --------------------------------------------------------------------------------------------------


class NetView:
    """Where a coupler network reads its input inside the current primal / tangent tensors."""

    def __init__(self, geom, cin, chan_off=0, chan_step=1, mask=None, live=None, probe=None):
        self.geom, self.cin, self.chan_off, self.chan_step, self.mask = geom, cin, chan_off, chan_step, mask
        #: probe front of a masked coupler (``probe_plan`` on the device: {"cls": int8, "ns": int, "probes": float32}) or None
        self.probe = probe
        #: checkerboard couplers: {"parity": 1 | 2, "act_idx": int32 map (hid * HW/2,) gathering the live pixels of a (hid, H, W)
        #: activation} -- the network's output is read at the pixels with (row + col) % 2 == parity - 1 only (net_tangent)
        self.live = live


class Geometry:
    """Shape of the tensor an ACL acts on: image (C, H, W) or flat (F,)."""

    def __init__(self, shape):
        self.shape = tuple(int(s) for s in shape)
        self.image = len(self.shape) == 3
        if self.image:
            self.C, self.H, self.W = self.shape
            self.HW = self.H * self.W
        else:
            assert len(self.shape) == 1
            self.C, self.H, self.W, self.HW = self.shape[0], 1, 1, 1
        self.N = int(np.prod(self.shape))


def _resnet_parts(net):
    body = net.module
    blocks = [m for m in body if hasattr(m, "conv1")]
    convs = [m for m in body if isinstance(m, nn.Conv2d)]
    return convs[0], blocks, convs[-1]


def net_primal(net, z, view, need_acts=True):
    """Primal forward of a coupler network on the current tensor ``z`` (B, *geom.shape).
    Returns (y (B, cout, ...), g or None, acts: activation tensors the tangent pass differentiates through;
    ``need_acts=False`` (encode pass, sampling) skips preparing them; the other forms of a ResNet coupler: CouplerPlan.acts)."""
    geo, B, dev = view.geom, z.shape[0], z.device
    if net.kind == "resnet":
        conv0, blocks, convf = _resnet_parts(net)
        hid, cout, H, W, HW = conv0.out_channels, convf.out_channels, geo.H, geo.W, geo.HW
        new = lambda c: torch.empty(B, c, H, W, dtype=torch.float32, device=dev)
        a = new(hid)
        conv_primal(z, view.chan_off * HW, geo.C * HW, view.chan_step * HW, 1, conv0.weight, 9, None, a, hid * HW, HW, 1,
                    B, view.cin, hid, H, W, imode=F_RAW if view.mask is not None else F_NONE, mask=view.mask, f_c=HW, f_px=1)
        plan = resnet_coupler_plan(net, view, B, None, need_acts)
        if plan.grouped:
            return _resnet_primal_grouped(net, blocks, convf, a, B, hid, cout, H, W, plan)
        acts = [a]
        for blk in blocks:
            c1 = new(hid)
            conv_primal(a, 0, hid * HW, HW, 1, blk.conv1.weight, 9, blk.conv1.bias, c1, hid * HW, HW, 1, B, hid, hid, H, W,
                        imode=F_RELU)
            a2 = new(hid)
            conv_primal(c1, 0, hid * HW, HW, 1, blk.conv2.weight, 9, blk.conv2.bias, a2, hid * HW, HW, 1, B, hid, hid, H, W,
                        imode=F_RELU, res=a)
            acts += [c1, a2]
            a = a2
        y, g = new(cout), new(cout)
        conv_primal(a, 0, hid * HW, HW, 1, convf.weight, 1, convf.bias, y, cout * HW, HW, 1, B, hid, cout, H, W,
                    imode=F_RELU, omode=O_STANH, sw=net.weights.detach().reshape(-1), sb=net.bias.detach().reshape(-1), g=g)
        return y, g, acts
    # MLP: pixels = batch samples, channels = features
    lins = [m for m in net if isinstance(m, nn.Linear)]
    F_in = geo.C
    h, h_c, h_px, h_off, cin = z, view.chan_step, F_in, view.chan_off, view.cin
    acts = []
    for i, lin in enumerate(lins):
        last = i == len(lins) - 1
        out = torch.empty(B, lin.out_features, dtype=torch.float32, device=dev)
        conv_primal(h, h_off, 0, h_c, h_px, lin.weight, 1, lin.bias, out, 0, 1, lin.out_features, 1, cin, lin.out_features,
                    1, B, omode=O_NONE if last else O_TANH)
        if not last:
            acts.append(out)
        h, h_c, h_px, h_off, cin = out, 1, lin.out_features, 0, lin.out_features
    return h, None, acts


def net_primal_zero_input(net, view, B, device):
    """(y, g), one row each, of a coupler network whose input is structurally ZERO -- the channels ``SplitDensity.pad_inputs``
    appended (split.py:50-52) feeding a coupler that passes exactly those through (acl.py:148-160): the output is the same for
    every sample, so ONE sample group runs (16 zero samples where the batch takes the sample-grouped kernels, 1 otherwise: the
    same kernels, hence the same bits, as the full batch) and the coupling kernels read it with sample stride 0.  Cached per
    parameter version and KernelConfig."""
    rows = 16 if B % 16 == 0 else 1
    params = list(net.parameters())

    def build():
        z0 = torch.zeros(rows, *view.geom.shape, dtype=torch.float32, device=device)
        y, g, _ = net_primal(net, z0, view, need_acts=False)
        return y[:1].clone(), (None if g is None else g[:1].clone())

    return DERIVED.get((id(params[0]), "zero-input", rows, cfg().primal, str(device)), params, build)


class GroupedActs(list):
    """Primal activations kept as (B/16, C, H, W, 16): 16 samples in the 16 column slots of the tangent kernels
    (supported as a factor source through ``f_group``, but slower to read than the standard layout)."""
    f_group = 16


class BitMask:
    """relu' of a hidden activation as one bit per (sample, pixel, channel): ``data`` (B, HW, C/8) uint8, the
    CMF_F_RELU_BITS layout (include/cmf_amd.h).  Written by the primal conv that produces the activation."""

    def __init__(self, B, HW, C, device):
        self.data = torch.empty(B, HW, C // 8, dtype=torch.uint8, device=device)
        self.np_bytes = HW * (C // 8)


class ActList(list):
    """Activations of a ResNet coupler kept for TRAINING: the elements are what the tangent pass and the reverse sweep read (the
    float a_0, relu' BitMasks of the hidden activations, the last activation as floats -- the "bits" form), and ``grouped`` holds
    ALL of them as the sample-grouped float tensors (B/16, C, HW, 16) the primal pass produced, which is what ``net_primal_backward``
    reads (else: 17 activations per coupler regrouped after the forward pass and back in the backward pass, 850 launches per step)."""
    grouped = None


def train_acts_mode(net, view, B, T=None, nc=None):
    """``need_acts`` for a training forward: "train" (ActList) where every consumer can work from bit masks and grouped floats,
    else True (per-sample float activations).  ``T`` = the tangent stack of the sweep that will read the activations, or ``nc``
    = its column slots when the sweep comes later (primal-only pass)."""
    return True if net.kind != "resnet" else resnet_coupler_plan(net, view, B, T.nc if T is not None else nc, "train-if-possible").acts


def _range_chain(on, nb, first):
    """The fp16 split kernel's input-range chain over a coupler's 2 ``nb`` hidden convs, forward or backward: word i = max |tensor i| (word
    0 by a reduction over ``first``, the others raised by the conv that stores the tensor, whose one reader is the next conv); a conv scales
    its input by the power of two that puts that maximum in [2^13, 2^14).  -> i: conv i's amax_in / amax_out keywords (none if not ``on``)."""
    if not on:
        return lambda i: {}
    rng = torch.zeros(2 * nb + 1, dtype=torch.float32, device=first.device)
    absmax(first, rng[0:1])
    return lambda i: dict(amax_in=rng[i:i + 1], amax_out=rng[i + 1:i + 2])


def _resnet_primal_grouped(net, blocks, convf, a0, B, hid, cout, H, W, plan):
    """Hidden 3x3 convs of the primal ResNet through the TANGENT conv kernels: the 16 column slots carry 16 samples (relu
    applied elementwise on load, bias as per-channel constant); ``plan`` (CouplerPlan) names the kernel, whether it writes relu'
    bit masks next to each activation, and the form the activations are handed out in."""
    HW, G, dev = H * W, B // 16, a0.device
    pn = GroupedBatch.image_strides(hid, HW)
    new = lambda: torch.empty(G * hid * HW * 16, dtype=torch.float32, device=dev)
    prec, bits, need_acts = plan.arith, plan.masks, plan.acts
    a = primal_regroup(a0, True)
    acts, masks = [a], []
    ax = _range_chain(prec == "f16x3", len(blocks), a)
    for k, blk in enumerate(blocks):
        c1, a2 = new(), new()
        m1, m2 = (BitMask(B, HW, hid, dev), BitMask(B, HW, hid, dev)) if bits else (None, None)
        mo = lambda m: dict(mask_out=m.data, mask_np=m.np_bytes) if m is not None else {}
        conv_tangent(a, 0, *pn, blk.conv1.weight, 9, c1, *pn, G, hid, hid, H, W, 16, fmode=F_SELF_RELU, bias=blk.conv1.bias,
                     precision=prec, **mo(m1), **ax(2 * k))
        conv_tangent(c1, 0, *pn, blk.conv2.weight, 9, a2, *pn, G, hid, hid, H, W, 16, fmode=F_SELF_RELU, bias=blk.conv2.bias,
                     res_t=a, precision=prec, **mo(m2), **ax(2 * k + 1))
        acts, masks, a = acts + [c1, a2], masks + [m1, m2], a2
    # 1x1 + ScaledTanh on the grouped tensor: a 1x1 conv does not care that "pixels" are (pixel, sample) pairs
    yg = torch.empty(G * cout * HW * 16, dtype=torch.float32, device=dev)
    gg = torch.empty_like(yg)
    conv_primal(a, 0, hid * HW * 16, HW * 16, 1, convf.weight, 1, convf.bias, yg, cout * HW * 16, HW * 16, 1, G, hid, cout,
                1, HW * 16, imode=F_RELU, omode=O_STANH, sw=net.weights.detach().reshape(-1), sb=net.bias.detach().reshape(-1), g=gg)
    y = primal_regroup(yg.view(G, -1), False).view(B, cout, H, W)
    g = primal_regroup(gg.view(G, -1), False).view(B, cout, H, W)
    if not need_acts:
        return y, g, None
    std_of = lambda t: primal_regroup(t.view(G, -1), False).view(B, hid, H, W)
    # Bit masks: nothing is regrouped but the last activation, which the 1x1 conv reads as floats.  Floats: the tangent pass reads
    # relu' per (channel, pixel) of ONE sample, and from the grouped layout every such read is its own 64-byte line (measured:
    # tangent convs 3.1 -> 4.5 ms); regrouping the 17 saved activations costs ~6 ms / elbo.
    out = [a0] + masks[:-1] + [std_of(acts[-1])] if bits else [a0] + [std_of(t) for t in acts[1:]]
    if need_acts == "train":                              # ActList: the same elements + the grouped floats
        out = ActList(out)
        out.grouped = acts
    return y, g, out


def _view_rows(T, view):
    """Compact copy of the rows of ``T`` a coupler network reads (``view``): cin channels, in T's layout."""
    if T.layout == "panel":
        HW = view.geom.HW
        rows = T.data[: T.B * T.N * T.nc].view(T.B, T.N // HW, HW * T.nc)[:, view.chan_off::view.chan_step][:, :view.cin]
        out = Tangent(T.B, view.cin * HW, T.nc, "panel", T.data.device)
    else:
        rows = T.data[: T.B * T.N * T.nc].view(T.N, T.B * T.nc)[view.chan_off::view.chan_step][:view.cin]
        out = Tangent(T.B, view.cin, T.nc, "fmajor", T.data.device)
    out.data.view(rows.shape).copy_(rows)
    return out


#: Switches of the work-skipping forms of a ResNet coupler's tangent sweep: ``TangentPlan`` says what each form is, ``resnet_tangent_plan``
#: reads them on every call.  False restores the launches the form replaced.
CHECKERBOARD_TAIL = True          # TangentPlan.tail "live", TangentPlan.compact (False: every pixel, rounds 1 - 4)
SKIP_DEAD_ROWS = True             # TangentPlan.filt
FOLD_HEAD = True                  # TangentPlan.tail "head"
FOLD_BLOCK = True                 # TangentPlan.tail "block"
PROBE_FRONT = True                # TangentPlan.front "probe"
SEED_RESIDUAL = True              # TangentPlan.front "seeded"
#: (H, W, cout) at which the folded block beat today's pair of launches by more than 3 x the run-to-run spread (profiles/fold_block.txt)
FOLD_BLOCK_SHAPES = ((28, 28, 2),)
#: (H, W, cin) at which the probe front beat today's launch by more than 3 x the run-to-run spread (profiles/probe_front.txt)
PROBE_FRONT_SHAPES = {(28, 28, 1)}
PROBE_CLASSES = 13


def probe_plan(mask):
    """Host plan of the probe front for a coupler whose network reads ``mask . v``; ``mask`` (cin, H, W) array, != 0 = an input row.
    Class of input row (c, r, col):  13 c + ((r - 5 col) mod 26 >> 1)  -- on either parity of the checkerboard these are the cosets
    of the lattice <(5, 1), (-1, 5)>, whose members are at Chebyshev distance >= 5 from each other, so a 5 x 5 window (the support of
    two stacked 3 x 3 convs) holds every class at most once.  Returns None unless that separation holds for THIS mask (checked by
    brute force: a mask that is not a checkerboard fails it), else a dict:
      cls (cin * H * W,) int8: the class, -1 where mask == 0;   ns = ceil(13 cin / 16): 16-column slices of probe columns;
      probes (cin * H * W, 16 ns) float32: the probe tangent in panel layout, column k = the sum of the unit impulses of class k."""
    mask = np.asarray(mask)
    if mask.ndim != 3:
        return None
    cin, H, W = mask.shape
    if not 1 <= cin <= 2:
        return None
    r, col = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cls = (np.mod(r - 5 * col, 2 * PROBE_CLASSES) >> 1)[None] + PROBE_CLASSES * np.arange(cin)[:, None, None]
    cls = np.where(mask != 0, cls, -1).astype(np.int8)
    # separation: every 5 x 5 window, clipped at the image border, holds each class at most once
    for r0 in range(H):
        for c0 in range(W):
            win = cls[:, max(r0 - 2, 0):r0 + 3, max(c0 - 2, 0):c0 + 3].reshape(-1)
            win = win[win >= 0]
            if len(np.unique(win)) != len(win):
                return None
    ns = (PROBE_CLASSES * cin + 15) // 16
    flat = cls.reshape(-1)
    probes = np.zeros((cin * H * W, 16 * ns), dtype=np.float32)
    rows = np.flatnonzero(flat >= 0)
    probes[rows, flat[rows]] = 1.0
    return {"cls": flat, "ns": ns, "probes": probes}


def probe_apply(R, r_np, r_px, T, t_off, t_np, t_c, t_px, cls, y, y_np, y_px, np_, cin, H, W, nc, ns, ymask=None):
    """``cmf_probe_apply`` (csrc/probe_front.hip): u0 from the probe responses ``R`` and the input rows of ``T``; ``ymask`` (a BitMask
    over the 64 output channels): rows whose bit is clear are neither computed nor written."""
    a = _lib.ProbeApplyArgs()
    a.r = _p(R); a.r_np, a.r_px = int(r_np), int(r_px)
    a.t = C.c_void_p(T.data_ptr() + 4 * int(t_off)); a.t_np, a.t_c, a.t_px = int(t_np), int(t_c), int(t_px)
    a.cls = _p(cls)
    a.y = _p(y); a.y_np, a.y_px = int(y_np), int(y_px)
    if ymask is not None:
        a.ymask, a.ymask_np = _p(ymask.data), int(ymask.np_bytes)
    a.np, a.cin, a.H, a.W, a.nc, a.ns = int(np_), int(cin), int(H), int(W), int(nc), int(ns)
    launch = lambda: _lib.check(_lib.load().cmf_probe_apply(C.byref(a), _stream()), "cmf_probe_apply")

    def cost():
        # <= 13 cin FMAs per output element; u0 is written and R read once (counted whole: the live fraction is data)
        px = float(H) * W * np_
        return 2.0 * PROBE_CLASSES * cin * 64 * nc * px, 4.0 * px * 64 * (nc + 16 * ns)
    return _timed(f"probe_apply_ci{cin}", cost, launch)


def seed_plane(H, W):
    """Floats per column plane of the seed panel: the zero-bordered image plus the one float a lane reads past its last row."""
    return ((H + 2) * (W + 2) + 1 + 3) // 4 * 4


def seed_panel(T, view, H, W):
    """``cmf_seed_panel``: mask . v of a one-channel coupler input as (B, nc, seed_plane) fp32 with an exact-zero border -- what the
    seeded-residual launch forms block 0's residual from.  ``T`` panel layout, read through ``view``."""
    assert T.layout == "panel" and view.cin == 1
    B, nc, HW, col = T.B, T.nc, H * W, seed_plane(H, W)
    out = torch.empty(B * nc * col, dtype=torch.float32, device=T.data.device)
    v = C.c_void_p(T.data.data_ptr() + 4 * int(view.chan_off * HW * nc))
    launch = lambda: _lib.check(_lib.load().cmf_seed_panel(v, T.t_b, nc, _p(view.mask), _p(out), nc * col, col, B, H, W, nc, _stream()),
                                "cmf_seed_panel")
    _timed("seed_panel", lambda: (0.0, 4.0 * B * nc * (col + HW)), launch)
    return dict(panel=out, np=nc * col, col=col)


def seed_pack_host(w):
    """Host restatement of ``cmf_pack_seed_weight`` (tests): ``w`` (64, 1, 3, 3) float32 array -> float32 (4, 64, 4), [co tile][lane =
    16 kq + co % 16][j]: tap 3 kq + j of channel 16 tile + co % 16 for kq, j < 3, zero otherwise."""
    w = np.asarray(w, dtype=np.float32).reshape(64, 9)
    out = np.zeros((4, 64, 4), dtype=np.float32)
    for kq in range(3):
        for j in range(3):
            out[:, 16 * kq:16 * kq + 16, j] = w[:, 3 * kq + j].reshape(4, 16)
    return out


def seed_panel_index(H, W):
    """Host restatement of ``cmf_seed_panel``'s index map (tests): int array (seed_plane,), element q of a column plane = the image
    pixel it holds, -1 on the zero border and in the padding."""
    idx = np.full(seed_plane(H, W), -1, dtype=np.int64)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    idx[((r + 1) * (W + 2) + c + 1).reshape(-1)] = (r * W + c).reshape(-1)
    return idx


def _seed_pack(conv0, dev):
    """conv0's weight (64, 1, 3, 3) as the B operands of the seed K-step (``cmf_pack_seed_weight``): a function of the weight
    alone, cached per parameter version like ``_probe_hidden``."""
    def build():
        w = conv0.weight.detach().contiguous()
        assert tuple(w.shape) == (64, 1, 3, 3) and w.dtype == torch.float32
        out = torch.empty(4096, dtype=torch.uint8, device=dev)
        _lib.check(_lib.load().cmf_pack_seed_weight(_p(w), _p(out), _stream()), "cmf_pack_seed_weight")
        return out

    return DERIVED.get((id(conv0.weight), "seed-residual", str(dev)), [conv0.weight], build)


def _block_pack(weight, dev):
    """The last block's conv1 weight (64, 64, 3, 3) as the pre-split B fragments of the folded block's coefficient build
    (``cmf_pack_block_weight``): a function of the weight alone, cached per parameter version like ``_seed_pack``."""
    def build():
        w = weight.detach().contiguous()
        assert tuple(w.shape) == (64, 64, 3, 3) and w.dtype == torch.float32
        n = C.c_longlong(0)
        _lib.check(_lib.load().cmf_pack_block_weight(None, None, C.byref(n), None), "pack size")
        out = torch.empty(n.value, dtype=torch.uint8, device=dev)
        _lib.check(_lib.load().cmf_pack_block_weight(_p(w), _p(out), None, _stream()), "cmf_pack_block_weight")
        return out

    return DERIVED.get((id(weight), "fold-block", str(dev)), [weight], build)


def _probe_hidden(conv0, view, plan, H, W, hid, dev):
    """conv0's tangent of the probe columns, (1, HW, ns, hid, 16) slice-major: a function of conv0's weight and the mask alone, so it is
    computed for ONE sample per parameter version (the thin kernel's arithmetic per element does not depend on the batch) and block
    0's conv1 reads it with sample stride 0."""
    HW, ncp = H * W, 16 * plan["ns"]

    def build():
        out = torch.empty(HW * hid * ncp, dtype=torch.float32, device=dev)
        conv_tangent(plan["probes"], 0, view.cin * HW * ncp, HW * ncp, ncp, conv0.weight, 9, out, hid * HW * ncp, 16, hid * ncp,
                     1, view.cin, hid, H, W, ncp, fmode=F_RAW, f=view.mask, f_np=0, f_ci=HW, f_px=1, y_sl=hid * 16)
        return out

    return DERIVED.get((id(conv0.weight), "probe-front", H, W, view.cin, str(dev)), [conv0.weight], build)


def probe_front(conv0, conv1, T, view, plan, factor, ymask, scratch, u, H, W):
    """u_0 = conv1(relu'(a_0) . conv0(mask . v)) of a 64-channel coupler through the probe columns of ``plan``: conv1 on
    conv0(probes) -- today's block-0 launch with nc = 16 ns, the same factor (``factor``: conv_tangent's f / fmode keywords) and the
    same store filter ``ymask`` -- writes the responses R into ``scratch`` (>= B * HW * 64 * 16 ns floats), and the apply kernel
    turns R and the input rows of ``T`` (panel layout, read through ``view``) into ``u`` (slice-major, rows with a clear bit
    untouched)."""
    B, nc, HW, hid, dev = T.B, T.nc, H * W, conv1.out_channels, T.data.device
    assert hid == 64 and T.layout == "panel"
    ncp = 16 * plan["ns"]
    conv_tangent(_probe_hidden(conv0, view, plan, H, W, hid, dev), 0, 0, 16, hid * ncp, conv1.weight, 9, scratch,
                 hid * HW * ncp, 16, hid * ncp, B, hid, hid, H, W, ncp, x_sl=hid * 16, y_sl=hid * 16, ymask=ymask, **factor)
    probe_apply(scratch, hid * HW * ncp, hid * ncp, T.data, view.chan_off * HW * nc, T.t_b, view.chan_step * HW * nc, nc,
                plan["cls"], u, hid * HW * nc, hid * nc, B, view.cin, H, W, nc, plan["ns"], ymask=ymask)


class TangentPlan(NamedTuple):
    """The launch set of one ResNet coupler's tangent sweep: ``resnet_tangent_plan`` decides, ``_resnet_tangent`` executes.  Anything
    but the plain form is evaluation only, on the split-precision kernel, for a network of whole 64-channel groups."""
    #: a block's conv1 gets c1's bit mask as its store filter.  A split-precision launch that takes relu' from a BitMask does not fetch
    #: the (channel, pixel) rows of its input whose bit is clear, and ``u``, the output of a block's conv1, has exactly one reader -- that
    #: block's conv2 in whichever form, through relu'(c1) -- so conv1 leaves those rows unwritten (they hold whatever the buffer held).
    #: The invariant: *a tensor with unwritten rows is only ever read by a launch that does not fetch those rows*.  Training keeps
    #: full stores: ``net_cotangent`` and the weight gradients read the saved ``u``.
    filt: bool
    #: how block 0 gets h_0 and u_0.  "plain": the thin conv0 launch, then conv1 on every column.  "probe": conv1 on one probe column per
    #: input class (13 per input channel) and the apply kernel form u_0 (csrc/probe_front.hip); h_0 is still the thin launch's.  "seeded":
    #: the probe front, and h_0 is never written -- block 0's conv2, its only reader, forms it from a one-channel seed panel.
    front: str
    #: how the last block reaches the network's output.  "plain": conv1, conv2, the 1x1 conv.  "live": a checkerboard layer reads (s, t,
    #: s-dot, t-dot) at its (1 - mask) pixels alone (acl.py:48-66) and the 1x1 conv is pointwise, so conv2 (with its residual read) and the
    #: 1x1 conv (on a gathered last activation) run on those pixels only.  "head": conv2 and the 1x1 conv as ONE fp32 launch that never
    #: forms h_K (csrc/conv_head.hip).  "block": that launch takes in conv1 too -- no conv1 launch, no ``u`` (csrc/conv_block_head.hip).
    tail: str
    #: the returned stack holds the live pixels only, (B, cout * HW/2, nc), pixel (row, col) at row * W/2 + col // 2 (``Tangent.compact``).
    #: Always under "live"; under "head" / "block" it follows CHECKERBOARD_TAIL alone, the same arithmetic per pixel either way (that
    #: switch stays bit-neutral: the full form is no speed claim).
    compact: bool


def resnet_tangent_plan(net, view, nc, layout, acts, training):
    """The TangentPlan of a ResNet coupler ``net`` read through ``view`` for a sweep of ``nc`` column slots in ``layout`` over the
    primal activations ``acts``; ``training``: the sweep saves its tangents.  Host logic on shapes, types and the module switches (read
    on every call) only: no device, no launch, no allocation."""
    conv0, blocks, convf = _resnet_parts(net)
    hid, cout, nb, H, W = conv0.out_channels, convf.out_channels, len(blocks), view.geom.H, view.geom.W
    # every form below belongs to the split kernel (whose shapes have an even W) and to evaluation: training keeps every tensor
    if training or hid % 64 or not _use_bf16x3(9, hid, W, False, H, hid):
        return TangentPlan(False, "plain", "plain", False)
    filt = bool(SKIP_DEAD_ROWS)
    # the other forms replace launches of a block and read the activations in the standard layout
    if nb == 0 or getattr(acts, "f_group", 1) != 1:
        return TangentPlan(filt, "plain", "plain", False)
    bits, live = (lambda i: isinstance(acts[i], BitMask)), view.live is not None
    # folded head, checkerboard couplers only: on every pixel of a 14 x 14 image the folded launch did not beat the two launches by
    # more than their own run-to-run spread (profiles/fold_head.txt), so the split-channel couplers keep them
    head = FOLD_HEAD and live and hid == 64 and cout <= 8 and nc % 16 == 0 and bits(2 * nb - 1)
    # folded block: block 0 belongs to the probe front and the seeded residual, hence two blocks or more
    block = head and FOLD_BLOCK and nb >= 2 and bits(2 * nb - 2) and (H, W, cout) in FOLD_BLOCK_SHAPES
    tail = "block" if block else "head" if head else "live" if CHECKERBOARD_TAIL and live else "plain"
    front, probe = "plain", view.probe
    if (PROBE_FRONT and probe is not None and hid == 64 and view.mask is not None and layout == "panel" and nc % 16 == 0
            and nc > 16 * probe["ns"] and (H, W, view.cin) in PROBE_FRONT_SHAPES):
        # seeded residual: under the probe front h_0 has ONE reader, block 0's conv2.  With one block that reader is the folded head,
        # which takes h as a tensor: that coupler keeps the thin launch
        front = "seeded" if SEED_RESIDUAL and view.cin == 1 and nb >= 2 and bits(1) else "probe"
    return TangentPlan(filt, front, tail, bool(CHECKERBOARD_TAIL and live))


class CouplerPlan(NamedTuple):
    """What a training step's other passes do with one ResNet coupler: ``resnet_coupler_plan`` decides, ``net_primal``, ``net_cotangent``
    and ``net_primal_backward`` execute.  Two things stay with the data and the launch on purpose: what the reverse sweep does with the
    activations it is actually HANDED (a BitMask as it is, floats through ``relu_bits``, also where a caller forced floats), and the
    per-launch gate inside ``conv_tangent`` / ``conv_tangent_wgrad``, which has the last word on the kernel."""
    #: primal pass: the hidden convs run on the tangent kernels, 16 samples in the column slots; else per sample on ``conv_primal``
    grouped: bool
    #: their arithmetic: KernelConfig.primal, or "f32" where the split kernels do not take the width -- they work on whole 64-channel
    #: groups (fp16) and fetch the bias of ONE group per launch (cmf_conv_tangent_f16x3 returns CMF_EINVAL for a bias with cout > 64)
    arith: str
    #: they write relu' bit masks next to each activation, 1/32 of the bytes (the bf16 split kernel writes none)
    masks: bool
    #: what ``net_primal`` hands out.  False: nothing (encode pass, sampling).  True: floats in the standard layout.  "bits": the float a_0,
    #: BitMasks of the hidden activations, the last activation as floats (the 1x1 conv reads those).  "train": an ActList, the same elements
    #: (floats without ``masks``) plus the grouped floats.  Requested as one of these, as "sweep" ("bits" for the split-precision tangent
    #: sweep, which reads relu' from masks, else True) or as "train-if-possible" ("train" where every consumer works from bit masks and
    #: grouped floats: groups of 32 samples, a split reverse sweep whose weight gradients take bits; else True)
    acts: object
    #: reverse sweep: the hidden transposed convs run on the split-precision kernel when the forward ones do -- no input factor, relu' as
    #: an output BIT MASK, cotangents slice-major like the forward tangents; else fp32 with float factors
    split: bool
    #: its hidden weight gradients take relu' as bit masks (the split kernel: column pairs; the fp32 one reads floats)
    wgrad_bits: bool
    #: primal backward: samples the batch is padded to.  32: the split-precision weight-gradient kernel contracts column PAIRS of 16, so
    #: two sample groups are presented as the two slices of one 32-column "sample" (slice stride = group stride)
    multiple: int
    #: its 2 K hidden weight (and bias) gradients go out TOGETHER: one alone would leave most of the chip idle -- at a training shard's 2 -
    #: 4 sample groups 28 - 56 image rows for 256 persistent workgroups (13.7 ms in 320 launches per C3 step at 64 samples)
    batched: bool
    #: its hidden data-gradient convs run the fp16 split kernel's backward form, with an input-range chain of its own
    bwd16: bool


def resnet_coupler_plan(net, view, B, nc=None, need_acts=True):
    """The CouplerPlan of a ResNet coupler ``net`` read through ``view`` on ``B`` samples; ``nc``: column slots of the sweep that reads
    the activations (None: a primal-only pass), ``need_acts``: the requested activation form (CouplerPlan.acts).  Host logic on shapes
    and the calling thread's KernelConfig (read on every call) only: no device, no launch, no allocation."""
    hid, H, W = _resnet_parts(net)[0].out_channels, view.geom.H, view.geom.W
    tangent, primal = cfg().tangent, cfg().primal
    tiles, whole = _shape_ok_bf16x3(9, hid, W, False, H, hid), hid % 64 == 0
    grouped = B % 16 == 0 and tiles
    arith = "f32" if (primal == "f16x3" and not whole) or hid > 64 else primal
    split = tangent == "bf16x3" and tiles and whole
    wgrad_bits = split and nc is not None and nc % 32 == 0
    if need_acts == "sweep":
        need_acts = "bits" if tangent == "bf16x3" else True
    if need_acts == "train-if-possible":
        need_acts = "train" if (B % 32 == 0 and tiles and whole and primal != "bf16x3" and (nc is None or wgrad_bits)) else True
    masks = grouped and need_acts in ("bits", "train") and arith != "bf16x3"
    if (need_acts == "bits" and not masks) or (need_acts == "train" and not grouped):
        need_acts = True                                  # floats are all the bf16 split kernel and the per-sample convs leave
    pair = tangent == "bf16x3" and whole                  # (the weight-gradient kernel: whatever the image's shape)
    batched = pair and hid == 64 and (B + 31) // 32 * H < 256
    return CouplerPlan(grouped, arith, masks, need_acts, split, wgrad_bits, 32 if pair else 16, batched, primal == "f16x3" and whole and tiles)


def net_tangent(net, T, view, acts, transpose_packs=False, save=None):
    """Push all Jacobian columns of ``T`` through the coupler network; returns the raw tangent of the network's pre-activation output
    (the ScaledTanh derivative ``g`` is applied by acl_tangent).  ``save`` (a list, training): the input tangent of every conv / linear
    layer is kept and appended, in forward order (the network's own input as a compact copy of the rows it reads), for
    ``net_cotangent(..., saved=, grads=)``.  Which launches a ResNet coupler gets, and what they may leave unwritten: ``TangentPlan``."""
    if save is not None:
        save.append(_view_rows(T, view))
    return (_resnet_tangent if net.kind == "resnet" else _mlp_tangent)(net, T, view, acts, save)


def _resnet_tangent(net, T, view, acts, save):
    """``net_tangent`` of a ResNet coupler: the launches its TangentPlan names, in forward order."""
    geo, B, nc, dev = view.geom, T.B, T.nc, T.data.device
    conv0, blocks, convf = _resnet_parts(net)
    hid, cout, H, W, HW, nb = conv0.out_channels, convf.out_channels, geo.H, geo.W, geo.HW, len(blocks)
    plan = resnet_tangent_plan(net, view, nc, T.layout, acts, save is not None)
    new = lambda c: Tangent(B, c * HW, nc, "panel", dev)
    # Hidden tangents live SLICE-MAJOR, [sample][pixel][16-column slice][channel][16]: the 16 channels x 16 columns an MFMA wave stores
    # (or reads as residual) per instruction are then one contiguous KiB instead of sixteen 64-byte pieces in sixteen channel planes --
    # that access shape ran at 13 B/clk/CU against 48 (tools/ubench/curate2.py) and was the 15k-cycle tail of every work item.  Only
    # the kernels' strides know about it.
    hd, hsl = (hid * HW * nc, 16, hid * nc), hid * 16    # (np, chan, px) strides, slice stride
    fg = getattr(acts, "f_group", 1)                     # primal activations: (B,C,H,W) or (B/16,C,H,W,16)
    fs = dict(f_np=hid * HW * fg, f_ci=HW * fg, f_px=fg, f_group=fg)
    # relu' source of a hidden conv: float activations, or the bit mask the primal pass wrote (BitMask)
    fk = lambda t: dict(fmode=F_RELU_BITS, f=t.data, f_np=t.np_bytes) if isinstance(t, BitMask) else dict(fmode=F_RELU, f=t, **fs)

    def folded(x, blk, factor, **kw):
        """The last block's conv2 and the 1x1 conv as one launch from ``x`` to the network's output, compact or full."""
        HWo = HW // 2 if plan.compact else HW
        yt = Tangent(B, cout * HWo, nc, "panel", dev, compact=plan.compact)
        conv_tangent(x.data, 0, *hd, blk.conv2.weight, 9, yt.data, cout * HWo * nc, HWo * nc, nc, B, hid, hid, H, W, nc, x_sl=hsl,
                     live=view.live["parity"] if plan.compact else 0, **kw, **factor)
        return yt

    u, h2, h = new(hid), new(hid), None
    if plan.front != "seeded":
        h = new(hid)
        conv_tangent(T.data, view.chan_off * HW * nc, T.t_b, view.chan_step * HW * nc, nc, conv0.weight, 9, h.data, *hd,
                     B, view.cin, hid, H, W, nc, fmode=F_RAW if view.mask is not None else F_NONE, f=view.mask, f_np=0,
                     f_ci=HW, f_px=1, y_sl=hsl)
    for k, blk in enumerate(blocks):
        a_in, c1, last = acts[2 * k], acts[2 * k + 1], k + 1 == nb
        ym = c1 if plan.filt and isinstance(c1, BitMask) else None
        if last and plan.tail == "block":
            return folded(h, blk, fk(a_in), head=dict(weight=convf.weight, act=acts[-1], conv1=dict(weight=blk.conv1.weight, mask=c1)))
        if k == 0 and plan.front != "plain":
            # the responses go through h2's buffer: free until conv2 writes it, after the apply kernel has read them
            probe_front(conv0, blk.conv1, T, view, view.probe, fk(a_in), ym, h2.data, u.data, H, W)
        else:
            conv_tangent(h.data, 0, *hd, blk.conv1.weight, 9, u.data, *hd, B, hid, hid, H, W, nc, x_sl=hsl, y_sl=hsl, **fk(a_in),
                         ymask=ym)
        if k == 0 and plan.front == "seeded":
            sd = seed_panel(T, view, H, W)
            conv_tangent(u.data, 0, *hd, blk.conv2.weight, 9, h2.data, *hd, B, hid, hid, H, W, nc, x_sl=hsl, y_sl=hsl,
                         seed=dict(sd, pack=_seed_pack(conv0, dev)), **fk(c1))
            h, h2 = h2, new(hid)
            continue
        if last and plan.tail == "head":
            return folded(u, blk, fk(c1), res_t=h.data, res_np=hd[0], head=dict(weight=convf.weight, act=acts[-1]))
        if last and plan.tail == "live":
            # the last hidden conv at the live pixels only, stored compactly; its residual read at those pixels of the full h
            HWc = HW // 2
            hc = Tangent(B, hid * HWc, nc, "panel", dev)
            conv_tangent(u.data, 0, *hd, blk.conv2.weight, 9, hc.data, hid * HWc * nc, 16, hid * nc, B, hid, hid, H, W, nc,
                         res_t=h.data, res_np=hd[0], x_sl=hsl, y_sl=hsl, live=view.live["parity"], **fk(c1))
            a_last = gather_primal(acts[-1], view.live["act_idx"], hid * HWc)         # relu' source of the 1x1 conv, compact too
            yt = Tangent(B, cout * HWc, nc, "panel", dev, compact=True)
            conv_tangent(hc.data, 0, hid * HWc * nc, 16, hid * nc, convf.weight, 1, yt.data, cout * HWc * nc, HWc * nc, nc, B, hid,
                         cout, H, W // 2, nc, fmode=F_RELU, f=a_last, x_sl=hsl, f_np=hid * HWc, f_ci=HWc, f_px=1)
            return yt
        conv_tangent(u.data, 0, *hd, blk.conv2.weight, 9, h2.data, *hd, B, hid, hid, H, W, nc, res_t=h.data, x_sl=hsl,
                     y_sl=hsl, **fk(c1))
        if save is not None:                              # keep h_k and u_k: no ping-pong reuse
            save += [h, u]
            h, u, h2 = h2, new(hid), new(hid)
        else:
            h, h2 = h2, h
    if save is not None:
        save.append(h)
    yt = new(cout)
    conv_tangent(h.data, 0, *hd, convf.weight, 1, yt.data, cout * HW * nc, HW * nc, nc, B, hid, cout, H, W, nc, fmode=F_RELU,
                 f=acts[-1], x_sl=hsl, **fs)
    return yt


def _mlp_tangent(net, T, view, acts, save):
    B, nc, dev = T.B, T.nc, T.data.device
    lins = [m for m in net if isinstance(m, nn.Linear)]
    x_t, x_off, x_ci, cin = T.data, view.chan_off * B * nc, view.chan_step * B * nc, view.cin
    fmode, f, f_px = F_NONE, None, 0
    out = None
    for i, lin in enumerate(lins):
        out = Tangent(B, lin.out_features, nc, "fmajor", dev)
        conv_tangent(x_t, x_off, 0, x_ci, nc, lin.weight, 1, out.data, 0, B * nc, nc, 1, cin, lin.out_features, 1, B, nc,
                     fmode=fmode, f=f, f_np=0, f_ci=1, f_px=f_px)
        if i < len(acts):
            fmode, f, f_px = F_TANH, acts[i], lin.out_features
        x_t, x_off, x_ci, cin = out.data, 0, B * nc, lin.out_features
        if save is not None and i + 1 < len(lins):
            save.append(out)
    return out


class GradPool(dict):
    """``grads`` dictionary (parameter -> gradient tensor) whose tensors are slices of ONE zero-filled buffer: a training step
    touches ~470 parameter tensors, and a ``zeros_like`` each was ~470 fill launches of 4 us per backward pass.  Only the parameters a
    backward pass actually reaches get an entry, exactly like the plain dict (parameters outside the graph keep ``grad = None``, as in
    the reference's autograd)."""

    def __init__(self, params, device):
        super().__init__()
        n = sum((p.numel() + 3) // 4 * 4 for p in params)             # 16-byte aligned slices
        self._pool = torch.zeros(max(n, 4), dtype=torch.float32, device=device)
        self._used = 0

    def zeros_for(self, weight):
        n = weight.numel()
        if self._used + n > self._pool.numel():                       # a parameter the pool was not sized for
            return torch.zeros_like(weight, dtype=torch.float32).contiguous()
        g = self._pool[self._used:self._used + n].view(weight.shape)
        self._used += (n + 3) // 4 * 4
        return g


def _grad_of(grads, weight):
    g = grads.get(weight)
    if g is None:
        g = grads[weight] = (grads.zeros_for(weight) if isinstance(grads, GradPool)
                             else torch.zeros_like(weight, dtype=torch.float32).contiguous())
    return g


def net_cotangent(net, YC, view, acts, Ct, saved=None, grads=None, cross=None):
    """Reverse sweep through the coupler network (the adjoint of ``net_tangent``): ``YC`` is the cotangent of the network's
    raw output; the cotangent of its input is ACCUMULATED into the rows of ``Ct`` the network reads (``view``).
    The adjoint of "factor, then conv" is "transposed conv, then factor": transposed / tap-flipped packs
    (``cmf_pack_weight(transpose=1)``) and the OUTPUT-side factor of ``cmf_conv_tangent`` (fp32 MFMA kernel), so every
    stored tensor is the true cotangent of a layer output.
    Training (``saved`` = the list ``net_tangent(save=)`` filled, ``grads`` = dict parameter -> gradient tensor): the weight
    gradient of every layer, ``dW += sum c_out (x) F x_in`` (``cmf_conv_tangent_wgrad``), is accumulated into ``grads``.
    Biases do not act on tangents and get no gradient here.  ``cross`` (MLP networks, a dict): receives, per hidden layer
    index, the cotangent of the primal tanh activation from the tangent rule's second-order term (``cmf_tanh_cross_terms``)."""
    geo, B, nc, dev = view.geom, Ct.B, Ct.nc, Ct.data.device
    f32 = dict(transpose=True, precision="f32")
    train = saved is not None
    assert not train or grads is not None
    if net.kind == "resnet":
        conv0, blocks, convf = _resnet_parts(net)
        hid, cout, H, W, HW = conv0.out_channels, convf.out_channels, geo.H, geo.W, geo.HW
        assert getattr(acts, "f_group", 1) == 1, "the reverse sweep reads per-sample activations"
        new = lambda c: Tangent(B, c * HW, nc, "panel", dev)
        pn = lambda c: (c * HW * nc, HW * nc, nc)          # (np, chan, px) strides of a panel with c channels
        hd, hsl = (hid * HW * nc, 16, hid * nc), hid * 16  # the forward pass's slice-major hidden layout (net_tangent)
        fa = dict(fo_np=hid * HW, fo_co=HW, fo_px=1, fomode=F_RELU)
        fr = dict(fmode=F_RELU, f_np=hid * HW, f_ci=HW, f_px=1)
        plan = resnet_coupler_plan(net, view, B, nc)
        split = plan.split                                 # (the skip connection is then the kernel's residual IN PLACE, below)
        cd, csl = (hd, hsl) if split else (pn(hid), 16)    # layout of the hidden cotangents
        if train:
            t_in, hs, us = saved[0], saved[1::2], saved[2::2]  # h_0 .. h_K, u_0 .. u_{K-1}
            assert len(hs) == len(blocks) + 1 and len(us) == len(blocks)
            # y = convf(relu'(a_last) . h_K)
            conv_tangent_wgrad(hs[-1].data, 0, *hd, YC.data, 0, *pn(cout), _grad_of(grads, convf.weight), 1, B, hid, cout, H, W, nc,
                               f=acts[-1], x_sl=hsl, **fr)
        # y = convf(relu'(a_last) . h)  ->  c_h = relu'(a_last) . convf^T(c_y)
        ch = new(hid)
        conv_tangent(YC.data, 0, *pn(cout), convf.weight, 1, ch.data, *cd, B, cout, hid, H, W, nc, fo=acts[-1], y_sl=csl, **fa, **f32)
        u, ch2 = new(hid), (None if split else new(hid))      # the in-place skip connection needs no second cotangent buffer
        # split kernels: relu' of both activations as bit masks (an ActList's, written by the primal pass, or made from the floats),
        # shared by the weight gradients (input factor) and the transposed convs (output mask); fp32: the float activations
        bits_of = lambda t: t if isinstance(t, BitMask) else relu_bits(t)
        tk = lambda act, bits: dict(fo=bits, transpose=True, x_sl=csl, y_sl=csl) if split else dict(fo=act, **fa, **f32)
        wf = lambda act, bits: dict(f=bits) if plan.wgrad_bits else dict(f=act, **fr)
        for k in reversed(range(len(blocks))):
            blk, a_in, c1 = blocks[k], acts[2 * k], acts[2 * k + 1]
            # h2 = h + conv2(relu'(c1) . u), u = conv1(relu'(a_in) . h):
            #   c_u = relu'(c1) . conv2^T(c_h2);   c_h = c_h2 + relu'(a_in) . conv1^T(c_u)
            b_c1, b_in = (bits_of(c1), bits_of(a_in)) if split else (None, None)
            assert split or not isinstance(c1, BitMask), "bit-mask activations need the split-precision reverse sweep"
            if train:
                conv_tangent_wgrad(us[k].data, 0, *hd, ch.data, 0, *cd, _grad_of(grads, blk.conv2.weight), 9, B, hid, hid, H, W,
                                   nc, x_sl=hsl, y_sl=csl, **wf(c1, b_c1))
            conv_tangent(ch.data, 0, *cd, blk.conv2.weight, 9, u.data, *cd, B, hid, hid, H, W, nc, **tk(c1, b_c1))
            if train:
                conv_tangent_wgrad(hs[k].data, 0, *hd, u.data, 0, *cd, _grad_of(grads, blk.conv1.weight), 9, B, hid, hid, H, W,
                                   nc, x_sl=hsl, y_sl=csl, **wf(a_in, b_in))
            # split: the skip connection IN PLACE, c_h += relu'(a_in) . conv1^T(c_u) -- the kernel starts its accumulators from c_h and
            # the lanes the mask switches off do not store (a separate accumulate pass cost 17 ms of a 235 ms step)
            dst = ch if split else ch2
            conv_tangent(u.data, 0, *cd, blk.conv1.weight, 9, dst.data, *cd, B, hid, hid, H, W, nc, res_t=ch.data, **tk(a_in, b_in))
            ch, ch2 = dst, (None if split else ch)
        # h0 = conv0(mask . v_in)  ->  Ct[view] += mask . conv0^T(c_h0)
        off = view.chan_off * HW * nc
        m = view.mask
        if train:
            conv_tangent_wgrad(t_in.data, 0, *pn(view.cin), ch.data, 0, *cd, _grad_of(grads, conv0.weight), 9, B, view.cin, hid,
                               H, W, nc, fmode=F_RAW if m is not None else F_NONE, f=m, f_np=0, f_ci=HW, f_px=1, y_sl=csl)
        conv_tangent(ch.data, 0, *cd, conv0.weight, 9, Ct.data, Ct.t_b, view.chan_step * HW * nc, nc, B, hid, view.cin, H, W, nc,
                     y_off=off, res_t=Ct.data, res_off=off, fo=m, fo_np=0, fo_co=HW, fo_px=1,
                     fomode=F_RAW if m is not None else F_NONE, x_sl=csl, **f32)
        return
    lins = [mod for mod in net if isinstance(mod, nn.Linear)]
    # x_i = W_i (phi_{i-1} . x_{i-1}), phi_0 = 1, phi_i = tanh'(h_i):  c_{i-1} = phi_{i-1} . W_i^T c_i  (output-side factor);
    # the chain ends unmasked, accumulated into the rows the network read.  dW_i = sum c_i (x) phi_{i-1} x_{i-1}.
    c_t, cin = YC.data, lins[-1].out_features
    for i in reversed(range(len(lins))):
        lin = lins[i]
        if train:
            xin = saved[i]
            fm = dict(fmode=F_TANH, f=acts[i - 1], f_np=0, f_ci=1, f_px=lin.in_features) if i > 0 else {}
            conv_tangent_wgrad(xin.data, 0, 0, B * nc, nc, c_t, 0, 0, B * nc, nc, _grad_of(grads, lin.weight), 1, 1, lin.in_features,
                               lin.out_features, 1, B, nc, **fm)
        if train and i > 0 and cross is not None:
            # training: the unmasked product first, then phi . (in place) together with the second-order term
            #   d h_{i-1} += -2 h_{i-1} sum_col (W_i^T c_i) x_{i-1}      (phi_{i-1} = 1 - h_{i-1}^2 is read by layer i's tangent rule)
            out = Tangent(B, lin.in_features, nc, "fmajor", dev)
            conv_tangent(c_t, 0, 0, B * nc, nc, lin.weight, 1, out.data, 0, B * nc, nc, 1, cin, lin.in_features, 1, B, nc, **f32)
            dh = torch.zeros_like(acts[i - 1])
            _lib.check(_lib.load().cmf_tanh_cross_terms(_p(out.data), out.t_b, out.t_r, _p(saved[i].data), saved[i].t_b, saved[i].t_r,
                                                        _p(acts[i - 1]), _p(dh), lin.in_features, B, nc, _stream()),
                       "cmf_tanh_cross_terms")
            cross[i - 1] = dh
            c_t, cin = out.data, lin.in_features
            continue
        if i == 0:
            off = view.chan_off * B * nc
            conv_tangent(c_t, 0, 0, B * nc, nc, lin.weight, 1, Ct.data, 0, view.chan_step * B * nc, nc, 1, cin, view.cin, 1, B, nc,
                         y_off=off, res_t=Ct.data, res_off=off, **f32)
        else:
            out = Tangent(B, lin.in_features, nc, "fmajor", dev)
            conv_tangent(c_t, 0, 0, B * nc, nc, lin.weight, 1, out.data, 0, B * nc, nc, 1, cin, lin.in_features, 1, B, nc,
                         fo=acts[i - 1], fo_np=0, fo_co=1, fo_px=lin.in_features, fomode=F_TANH, **f32)
            c_t, cin = out.data, lin.in_features


def net_primal_backward(net, z, view, acts, y, g, dy, dg, grads, dz):
    """Primal backward of a ResNet coupler network (training): given the cotangents ``dy`` of its output
    ``y = sw tanh(u) + sb`` and ``dg`` of the tangent multiplier ``g`` (from ``acl_cross_terms``; may be None), accumulates
    the gradients of every weight, bias and of the ScaledTanh parameters into ``grads`` and the cotangent of the rows of
    ``z`` the network read into ``dz``.  ``acts`` = what ``net_primal`` returned: per-sample floats (need_acts True), or an ActList
    ("train"), whose grouped floats are read as they are when the batch needs no padding.  Runs on the tangent-conv kernels with 16
    samples in the column slots (CouplerPlan.multiple, .batched, .bwd16): transposed packs with the per-column output factor
    (``CMF_F_SELF_RELU`` as fomode), ``cmf_conv_tangent_wgrad`` with the input's own relu, ``cmf_channel_sum`` for biases."""
    assert net.kind == "resnet", "MLP couplers: the tanh layers add second-order cross terms that are not built yet"
    geo, B, dev = view.geom, z.shape[0], z.device
    conv0, blocks, convf = _resnet_parts(net)
    hid, cout, H, W, HW = conv0.out_channels, convf.out_channels, geo.H, geo.W, geo.HW
    plan = resnet_coupler_plan(net, view, B)
    pair, batch_wgrads, use16 = plan.multiple == 32, plan.batched, plan.bwd16
    gb = GroupedBatch(B, dev, plan.multiple)
    G, grp = gb.G, gb.pack                                 # (B, C, H, W) -> flat grouped (G, C, HW, 16), zero-padded samples
    pn = lambda c: gb.image_strides(c, HW)
    new = lambda c: torch.empty(G * c * HW * 16, dtype=torch.float32, device=dev)
    gs = hid * HW * 16                                  # group stride = slice stride of a PAIR of groups: its strides and keywords
    pp, pk = (2 * gs, HW * 16, 16), dict(fmode=F_SELF_RELU, x_sl=gs, y_sl=gs)
    pending = []                                        # batch_wgrads: the hidden convs' operands, launched TOGETHER once all exist

    def flush_grads():
        parts = [list(zip(*pending[i:i + _lib.WGRAD_MAX_BATCH])) for i in range(0, len(pending), _lib.WGRAD_MAX_BATCH)]
        for xs, gys, dws, _ in parts:
            conv_tangent_wgrad_batched(list(xs), list(gys), list(dws), *pp, *pp, G // 2, hid, hid, H, W, 32, **pk)
        for _, gys, _, dbs in parts:                    # the hidden convs' bias gradients: one launch too
            channel_sum_batched(list(gys), *pn(hid), G, hid, HW, 16, list(dbs))

    def hidden_grads(x_g, gy_g, conv):                  # weight (3x3, hid -> hid, the input's own relu) and bias gradient
        dw, db = _grad_of(grads, conv.weight), _grad_of(grads, conv.bias)
        if batch_wgrads:
            return pending.append((x_g, gy_g, dw, db))  # the tensors stay alive until the flush
        if pair:
            conv_tangent_wgrad(x_g, 0, *pp, gy_g, 0, *pp, dw, 9, G // 2, hid, hid, H, W, 32, **pk)
        else:
            conv_tangent_wgrad(x_g, 0, *pn(hid), gy_g, 0, *pn(hid), dw, 9, G, hid, hid, H, W, 16, fmode=F_SELF_RELU)
        channel_sum(gy_g, *pn(hid), G, hid, HW, 16, db)

    tr = dict(transpose=True, precision="f32")
    self_fo = lambda t: dict(fo=t, fo_np=hid * HW * 16, fo_co=HW * 16, fo_px=16, fomode=F_SELF_RELU)
    du = stanh_backward(dy, dg, y, g, net.weights, net.bias, _grad_of(grads, net.weights).view(-1), _grad_of(grads, net.bias).view(-1))
    kept = getattr(acts, "grouped", None) if gb.Bp == B else None   # ActList: the forward pass's grouped tensors, no regrouping
    gact = lambda i: kept[i] if kept is not None else grp(acts[i])
    du_g, a_g = grp(du), gact(len(acts) - 1)
    # u = convf(relu(a_K)) + bf
    conv_tangent_wgrad(a_g, 0, *pn(hid), du_g, 0, *pn(cout), _grad_of(grads, convf.weight), 1, G, hid, cout, H, W, 16, fmode=F_SELF_RELU)
    channel_sum(du_g, *pn(cout), G, cout, HW, 16, _grad_of(grads, convf.bias))
    da = new(hid)
    conv_tangent(du_g, 0, *pn(cout), convf.weight, 1, da, *pn(hid), G, cout, hid, H, W, 16, **self_fo(a_g), **tr)
    # hidden 3x3 data-gradient convs: the fp16 split kernel's backward form with its own input-range chain, from max |da| on
    ax = _range_chain(use16, len(blocks), da)
    tr16 = lambda i: dict(transpose=True, precision="f16x3", **ax(i)) if use16 else tr
    for j, k in enumerate(reversed(range(len(blocks)))):
        blk = blocks[k]
        a_in, c1 = gact(2 * k), gact(2 * k + 1)
        # a' = a + conv2(relu(c1)) + b2,  c1 = conv1(relu(a)) + b1
        hidden_grads(c1, da, blk.conv2)
        dc1 = new(hid)
        conv_tangent(da, 0, *pn(hid), blk.conv2.weight, 9, dc1, *pn(hid), G, hid, hid, H, W, 16, **self_fo(c1), **tr16(2 * j))
        hidden_grads(a_in, dc1, blk.conv1)
        da2 = new(hid)
        conv_tangent(dc1, 0, *pn(hid), blk.conv1.weight, 9, da2, *pn(hid), G, hid, hid, H, W, 16, res_t=da, **self_fo(a_in), **tr16(2 * j + 1))
        da = da2
    flush_grads()
    # a_0 = conv0(mask . z[view])   (no bias)
    cin, m = view.cin, view.mask
    rows = z.reshape(B, geo.C, HW)[:, view.chan_off::view.chan_step][:, :cin]
    x0 = grp(rows)
    fm = dict(fmode=F_RAW, f=m, f_np=0, f_ci=HW, f_px=1) if m is not None else {}
    conv_tangent_wgrad(x0, 0, *pn(cin), da, 0, *pn(hid), _grad_of(grads, conv0.weight), 9, G, cin, hid, H, W, 16, **fm)
    dx0 = new(cin)
    fo = dict(fo=m, fo_np=0, fo_co=HW, fo_px=1, fomode=F_RAW) if m is not None else {}
    conv_tangent(da, 0, *pn(hid), conv0.weight, 9, dx0, *pn(cin), G, hid, cin, H, W, 16, **fo, **tr)
    dz.reshape(B, geo.C, HW)[:, view.chan_off::view.chan_step][:, :cin] += gb.unpack(dx0, cin * HW).view(B, cin, HW)


def mlp_primal_backward(net, z, view, acts, dy, grads, dz, dh_extra=None):
    """Primal backward of an MLP coupler network (2-D / tabular couplers and every low-dimensional prior flow) on the same
    kernels as the ResNet path: 16 samples ride in the 16 column slots of the tangent-conv kernels (``cmf_primal_regroup``), so
    per layer  dW += sum d (x) h  is ``cmf_conv_tangent_wgrad`` with taps = 1,  db  is ``cmf_channel_sum``,  W^T d  is
    ``cmf_conv_tangent`` on the transposed pack, and the tanh stage  d = (dh + extra) (1 - a^2)  is ``cmf_tanh_backward``.
    ``acts`` = the tanh outputs ``net_primal`` returned; ``dh_extra`` = the tangent pass's second-order terms
    (``net_cotangent(cross=)``).  Accumulates weight / bias gradients into ``grads`` and the input cotangent into ``dz``."""
    assert net.kind == "mlp" and view.mask is None
    lins = [m for m in net if isinstance(m, nn.Linear)]
    B, dev = z.shape[0], z.device
    gb = GroupedBatch(B, dev)
    G, grp, pn = gb.G, gb.pack, gb.strides                 # (B, F) -> (G, F, 16) as ONE image row of G "pixels", as the MLP tangent pass
    rows = z.reshape(B, -1)[:, view.chan_off::view.chan_step][:, :view.cin]
    hs = [grp(rows)] + [grp(a) for a in acts]              # input of every linear layer, grouped
    d_g = grp(dy.reshape(B, -1))
    lib = _lib.load()
    for i in reversed(range(len(lins))):
        lin = lins[i]
        cin, cout = lin.in_features, lin.out_features
        conv_tangent_wgrad(hs[i], 0, *pn(cin), d_g, 0, *pn(cout), _grad_of(grads, lin.weight), 1, 1, cin, cout, 1, G, 16)
        channel_sum(d_g, *pn(cout), 1, cout, G, 16, _grad_of(grads, lin.bias))
        dh_g = torch.empty(G * cin * 16, dtype=torch.float32, device=dev)
        conv_tangent(d_g, 0, *pn(cout), lin.weight, 1, dh_g, *pn(cin), 1, cout, cin, 1, G, 16, transpose=True, precision="f32")
        if i > 0:
            extra = grp(dh_extra[i - 1]) if dh_extra is not None and (i - 1) in dh_extra else None
            _lib.check(lib.cmf_tanh_backward(_p(dh_g), _p(hs[i]), _p(extra), dh_g.numel(), _p(dh_g), _stream()), "cmf_tanh_backward")
            d_g = dh_g
        else:
            dz.reshape(B, -1)[:, view.chan_off::view.chan_step][:, :view.cin] += gb.unpack(dh_g, cin)
