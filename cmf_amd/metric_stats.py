"""Dataset-level statistics of the pull-back metric G = J^T J: the batch-mean metric, the ranking of the latent
dimensions by mean g_kk and MACS, the mean absolute cosine similarity of the Jacobian columns -- the numbers the reference's
visualizer reports (visualizer.py:191-214, :305-317, :366, :381-397) from an autograd loop over 64 - 128 samples.  Here every
sample's G is already on the device; ``MetricStatistics.update`` streams batches through the decode sweep and one reduction
kernel (csrc/metric_stats.hip) into a flat float64 state, and nothing leaves the device before ``result()``.

    stats = cmf_amd.MetricStatistics(density)
    for x, _ in loader:
        stats.update(x.cuda())
    print(stats.result()["macs"])
"""
import torch

from . import engine as E
from .bijections import AffineBijection, AffineCouplingBijection, _ReshapingBijection
from .densities import ManifoldFlowHeadDensity, NonSquareHeadDensity

__all__ = ["MetricState", "MetricStatistics"]

COORDINATES = ("latent", "noise")


def metric_head(density, coordinates, what):
    """The one non-square head of ``density`` whose metric ``what`` ("metric statistics", ...) is about, after the checks every
    consumer of ``gram_batches`` makes in its constructor."""
    if coordinates not in COORDINATES:
        raise ValueError(f"coordinates must be one of {COORDINATES}, got {coordinates!r}")
    heads = [m for m in density.modules() if isinstance(m, NonSquareHeadDensity)]
    if len(heads) != 1:
        raise ValueError(f"{what} need a density with one non-square head, found {len(heads)}")
    if isinstance(heads[0], ManifoldFlowHeadDensity):
        raise NotImplementedError(f"{what} of the M-flow baseline head are not built (DESIGN 8)")
    prog = heads[0].program
    E.check_latent_width(prog.d)
    if coordinates == "noise":
        for m in prog.prior:
            if not isinstance(m, (AffineCouplingBijection, AffineBijection, _ReshapingBijection)):
                raise NotImplementedError(f"coordinates='noise': the tangent of the prior layer {type(m).__name__} is not built")
    return heads[0]


def gram_batches(density, head, x, coordinates, ident):
    """The Gram matrices of the samples of ``x``, sub-batch by sub-batch like the log-density path
    (``FlowProgram.TANGENT_BUDGET``): yields (i, j, jtj) with jtj (j - i, d, d) float32 the metric of x[i:j] in ``coordinates``,
    as ONE factorisation attempt leaves it (no jitter ever touches it).  Call under ``torch.no_grad()``; enqueues kernels only and
    leaves ``head.last_gram`` alone.  ``ident``: a dict the caller keeps between calls (the index vector of ``_prior_jacobian``)."""
    prog, B = head.program, x.shape[0]
    chunk = prog.tangent_chunk(B)
    for i in range(0, B, chunk):
        z_low = density.extract_latent(x[i:i + chunk], earliest_latent=False)
        eps = _prior_jacobian(head, z_low, ident) if coordinates == "noise" else None
        _, T = prog.decode(z_low, tangents=True, eps=eps)
        yield i, min(i + chunk, B), E.gram_cholesky(T, prog.d, 1).jtj


def _prior_jacobian(head, z_low, ident):
    """P = d z_low / d u (B, d, d) at u = prior(z_low): the prior layers in decode order on u with an identity-seeded tangent
    stack of d columns, under the head's KernelConfig."""
    prog, (B, d), dev = head.program, z_low.shape, z_low.device
    if ident.get("device") != dev:
        ident["device"], ident["index"] = dev, torch.arange(2 * d, dtype=torch.int32, device=dev)
    rows, tail = ident["index"][:d], ident["index"][d:]
    with E.scope(head.kernels):
        u = z_low.clone()
        for m in prog.prior:
            u = m.prior_encode(u)
        T = E.seed_tangent(B, d, E.ceil16(d), "fmajor", rows, d, dev)
        for m in reversed(prog.prior):
            if isinstance(m, AffineCouplingBijection):
                m.decode_(u, T, ncols=d)
            elif isinstance(m, AffineBijection):
                # z = (u - shift) e^{-log_scale}: the coupling update with no network tangent scales row f by e^{-s_f}
                y = torch.cat((m.shift.detach().reshape(1, d), m.log_scale.detach().reshape(1, d)), dim=1)
                E.acl_tangent(T, None, u, y, None, {"zi": rows, "ti": rows, "si": tail, "n": d})
                m.decode_(u)
            # (a reshaping layer of the flat prior is a view: FlowProgram's prior sweeps pass it by as well)
    return T.to_dense(d).contiguous()


class MetricState:
    """The running sums as ONE flat float64 tensor ``[S_G (d*d) | S_cos (d*d) | count | skipped]`` on any device: what
    ``engine.metric_stats_accumulate`` adds to, and everything that needs no kernel -- merging, the all-reduce, finalisation."""

    def __init__(self, d, device="cpu"):
        self.d = int(d)
        self.flat = torch.zeros(E.metric_stats_state_size(d), dtype=torch.float64, device=device)

    def reset(self):
        self.flat.zero_()

    def merge(self, other):
        """Add another state (another loader shard, another instance) to this one."""
        if other.d != self.d:
            raise ValueError(f"cannot merge metric statistics of latent dimension {other.d} into {self.d}")
        self.flat += other.flat.to(self.flat.device)
        return self

    def all_reduce(self, group=None):
        """Sum the state over the ranks of ``group``: ONE all-reduce of the flat tensor (the two counts ride along as doubles,
        exact up to 2^53 samples)."""
        import torch.distributed as dist
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
        return self

    def result(self):
        """Finalise on the host (one device-to-host copy of the flat state): a dict of float64 CPU tensors and Python numbers."""
        d, dd = self.d, self.d * self.d
        flat = self.flat.cpu()
        count, skipped = int(flat[2 * dd]), int(flat[2 * dd + 1])
        if count == 0:
            raise ValueError(f"metric statistics of no sample ({skipped} skipped): call update() first")
        mean_metric = flat[:dd].view(d, d) / count
        mean_cosine = flat[dd:2 * dd].view(d, d) / count
        mean_diagonal = torch.diagonal(mean_metric).clone()
        off = ~torch.eye(d, dtype=torch.bool)
        return {
            "count": count,
            "skipped": skipped,
            "mean_metric": mean_metric,
            "mean_diagonal": mean_diagonal,
            "mean_metric_normalized": mean_metric / mean_metric.abs().max(),          # v2, visualizer.py:213-214
            "mean_diagonal_normalized": mean_diagonal / mean_diagonal.abs().max(),    # v1, :205-206
            "mean_cosine": mean_cosine,
            "macs": float(mean_cosine.abs().mean()),                                  # :366, the diagonal included
            "macs_offdiag": float(mean_cosine.abs()[off].mean()) if d > 1 else 0.0,
            "ranking": torch.argsort(mean_diagonal.abs(), stable=True),               # :395, least prominent dimension first
        }


class MetricStatistics:
    """Streaming metric statistics of a non-square density.

    ``coordinates="latent"``: J = d x_hat / d z_low, the Jacobian the log-density path factorises.  ``"noise"``: the reference's
    coordinates, J P with P = d z_low / d u through the low-dimensional prior flow (visualizer.py:193-196 differentiates with
    respect to the earliest latent).  ``update(x)`` adds a batch and returns each sample's mean |cos_ij| over i != j (NaN for a
    sample whose metric has a non-positive or non-finite diagonal entry: counted in ``skipped``, added to nothing)."""

    def __init__(self, density, coordinates="latent"):
        self.density, self.head, self.coordinates = density, metric_head(density, coordinates, "metric statistics"), coordinates
        prog = self.head.program
        self.state = MetricState(prog.d, device=prog.tail.permutation.device)
        self._ident = {}

    # the state's own operations, so that a loop needs one object ------------------------------------
    def reset(self):
        self.state.reset()

    def merge(self, other):
        self.state.merge(other.state if isinstance(other, MetricStatistics) else other)
        return self

    def all_reduce(self, group=None):
        self.state.all_reduce(group)
        return self

    def result(self):
        return self.state.result()

    # ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, x):
        """Add the samples of ``x`` (the density's input; never modified, no dequantisation noise is drawn); returns (B,) float32
        on the device.  Sub-batches like the log-density path (``FlowProgram.TANGENT_BUDGET``); enqueues kernels only -- no copy
        to the host, no synchronisation -- and leaves ``head.last_gram`` alone."""
        E.require_gpu(x)
        macs = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        for i, j, jtj in gram_batches(self.density, self.head, x, self.coordinates, self._ident):
            E.metric_stats_accumulate(jtj, self.state.flat, sample_macs=macs[i:j])
        return macs
