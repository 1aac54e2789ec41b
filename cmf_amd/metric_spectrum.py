"""The spectrum of the pull-back metric G = J^T J, per sample and streamed over a data set: the eigenvalues
lambda_1 <= ... <= lambda_d of every sample's G (the squared singular values of its Jacobian), optionally the eigenvectors, and
from them the log-volume 1/2 sum_k log lambda_k, the 2-norm condition number, the participation ratio and the effective rank.
The decomposition is one kernel (csrc/gram_spectrum.hip: float64 Jacobi, one workgroup per sample) behind the decode sweep that
``MetricStatistics`` runs; nothing leaves the device before ``result()``.

    spectrum = cmf_amd.MetricSpectrum(density)
    for x, _ in loader:
        out = spectrum.update(x.cuda())                       # device tensors for this batch
        rank = cmf_amd.effective_rank(out["eigenvalues"], 1e-6)
    print(spectrum.result()["mean_log_eigenvalues"])
"""
import torch

from . import engine as E
from .metric_stats import gram_batches, metric_head

__all__ = ["SpectrumState", "MetricSpectrum", "effective_rank"]


def effective_rank(eigenvalues, rel_tol):
    """Per sample, the number of eigenvalues above ``rel_tol`` times the largest: (..., d) -> (...) int64.  A sample whose
    eigenvalues are NaN counts 0."""
    lam_max = eigenvalues.max(dim=-1, keepdim=True).values
    return (eigenvalues > rel_tol * lam_max).sum(dim=-1)


class SpectrumState:
    """The running sums as ONE flat float64 tensor ``[S_log (d) | S_lam (d) | S_pr | count | skipped]`` on any device: position
    by position over the ascending spectra of the valid samples, the sums of log lambda_k and of lambda_k, the sum of the
    participation ratios, and the numbers of samples counted and skipped."""

    def __init__(self, d, device="cpu"):
        self.d = int(d)
        self.flat = torch.zeros(2 * self.d + 3, dtype=torch.float64, device=device)

    def reset(self):
        self.flat.zero_()

    def merge(self, other):
        """Add another state (another loader shard, another instance) to this one."""
        if other.d != self.d:
            raise ValueError(f"cannot merge metric spectra of latent dimension {other.d} into {self.d}")
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
        d = self.d
        flat = self.flat.cpu()
        count, skipped = int(flat[2 * d + 1]), int(flat[2 * d + 2])
        if count == 0:
            raise ValueError(f"metric spectrum of no sample ({skipped} skipped): call update() first")
        mean_log = flat[:d] / count
        return {
            "count": count,
            "skipped": skipped,
            "mean_log_eigenvalues": mean_log,                       # exp of it: the geometric-mean spectrum
            "mean_eigenvalues": flat[d:2 * d] / count,
            "mean_participation_ratio": float(flat[2 * d]) / count,
            "mean_log_volume": 0.5 * float(mean_log.sum()),
        }


class MetricSpectrum:
    """Per-sample and streaming spectrum of the metric of a non-square density with latent dimension <= 128.

    ``coordinates`` as in ``MetricStatistics``: ``"latent"`` is J = d x_hat / d z_low, ``"noise"`` is J P through the
    low-dimensional prior flow.  ``update(x)`` decomposes the batch and adds its valid samples -- converged, smallest eigenvalue
    positive -- to the state; the others are counted in ``skipped`` and added to nothing.  ``vectors=True`` also returns the
    eigenvectors."""

    def __init__(self, density, coordinates="latent", vectors=False):
        self.density, self.head, self.coordinates = density, metric_head(density, coordinates, "metric spectra"), coordinates
        prog = self.head.program
        if prog.d > E.SPECTRUM_MAX_WIDTH:
            raise ValueError(f"latent_dimension = {prog.d}: the metric spectrum supports 1 <= latent_dimension <= "
                             f"{E.SPECTRUM_MAX_WIDTH} (DESIGN 9)")
        self.vectors = bool(vectors)
        self.state = SpectrumState(prog.d, device=prog.tail.permutation.device)
        self._ident = {}

    # the state's own operations, so that a loop needs one object ------------------------------------
    def reset(self):
        self.state.reset()

    def merge(self, other):
        self.state.merge(other.state if isinstance(other, MetricSpectrum) else other)
        return self

    def all_reduce(self, group=None):
        self.state.all_reduce(group)
        return self

    def result(self):
        return self.state.result()

    # ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, x):
        """Decompose the metric of every sample of ``x`` (the density's input; never modified, no dequantisation noise is drawn)
        and add the valid ones to the state.  Returns device tensors for the B samples: ``eigenvalues`` (B, d) float64 ascending,
        ``vectors`` (B, d, d) if requested, ``info`` and ``sweeps`` (B,) int32 (``engine.gram_spectrum``), ``log_volume`` (B,)
        = 1/2 sum_k log lambda_k (NaN unless the sample is valid), ``condition`` (B,) = lambda_max / lambda_min (+inf where
        lambda_min <= 0, NaN for a non-finite metric) and ``participation_ratio`` (B,) = (sum lambda)^2 / sum lambda^2.
        Sub-batches like the log-density path; enqueues kernels only -- no copy to the host, no synchronisation -- and leaves
        ``head.last_gram`` alone."""
        E.require_gpu(x)
        parts = [E.gram_spectrum(jtj, vectors=self.vectors)
                 for _, _, jtj in gram_batches(self.density, self.head, x, self.coordinates, self._ident)]
        cat = lambda name: getattr(parts[0], name) if len(parts) == 1 else torch.cat([getattr(p, name) for p in parts])
        out = summarize(cat("eigenvalues"), cat("info"))
        out["sweeps"] = cat("sweeps")
        if self.vectors:
            out["vectors"] = cat("vectors")
        accumulate(self.state.flat, out)
        return out


def summarize(eigenvalues, info):
    """The per-sample numbers ``MetricSpectrum.update`` returns, from ascending ``eigenvalues`` (B, d) float64 and ``info`` (B,):
    torch operations on whatever device holds them, no synchronisation."""
    lam_min, lam_max = eigenvalues[:, 0], eigenvalues[:, -1]
    valid = (info == 0) & (lam_min > 0)
    nan = torch.full_like(lam_min, float("nan"))
    safe = torch.where(valid[:, None], eigenvalues, torch.ones_like(eigenvalues))
    condition = torch.where(lam_min > 0, lam_max / lam_min, torch.full_like(lam_min, float("inf")))
    return {
        "eigenvalues": eigenvalues,
        "info": info,
        "valid": valid,
        "log_volume": torch.where(valid, 0.5 * safe.log().sum(1), nan),
        "condition": torch.where(info == 2, nan, condition),
        "participation_ratio": eigenvalues.sum(1) ** 2 / (eigenvalues * eigenvalues).sum(1),
    }


def accumulate(flat, out):
    """Add the valid samples of ``summarize``'s output to the flat state of a ``SpectrumState`` (masked float64 reductions on the
    device of the tensors)."""
    lam, valid = out["eigenvalues"], out["valid"]
    mask = valid[:, None]
    log_lam = torch.where(mask, lam, torch.ones_like(lam)).log()             # log 1 = 0 for a sample that does not count
    lam = torch.where(mask, lam, torch.zeros_like(lam))
    pr = torch.where(valid, out["participation_ratio"], torch.zeros_like(lam[:, 0]))
    n_valid = valid.sum().to(torch.float64)
    flat += torch.cat((log_lam.sum(0), lam.sum(0), torch.stack((pr.sum(), n_valid, valid.numel() - n_valid))))
