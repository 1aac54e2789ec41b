"""Shortest paths on the learned manifold: the geodesic of the pull-back metric between two inputs and its length.
Straight interpolation in the latent space is not that geodesic; ``ManifoldGeodesic`` relaxes a curve of ``points`` latents with
fixed ends by damped Gauss-Newton (Levenberg-Marquardt) steps on the energy E = N sum_i ||g(z_{i+1}) - g(z_i)||^2, started on the
straight latent line.  A step is one decode sweep over all points of all curves (x_hat, J), the Gram kernel (J_i^T J_i), the
cross-Gram kernel (J_i^T J_{i+1}) and one per-curve kernel (csrc/curve_step.hip: the gradient and the float64 solve of the block
tridiagonal normal equations); nothing leaves the device.

    geo = cmf_amd.ManifoldGeodesic(density, points=17)
    out = geo.connect(x0.cuda(), x1.cuda())
    out["length"], out["initial_length"]                 # in the head's input space, after and on the straight latent line
    out["path"]                                          # (B, points, *x_shape) in data space
"""
import torch

from . import engine as E
from .metric_stats import metric_head
from .projection import DAMPING_MAX, DAMPING_MIN, ManifoldProjector

__all__ = ["ManifoldGeodesic"]


class ManifoldGeodesic:
    """Damped Gauss-Newton relaxation of discretised curves on the manifold of a non-square density with latent dimension <= 128.

    A curve has ``points`` >= 3 latents; its ends stay where they are.  ``steps`` iterations per call; every curve carries its own
    damping lambda, started at ``damping``: a step is accepted iff its solve succeeded and it strictly lowers the energy, then
    lambda <- max(lambda ``down``, 1e-12); otherwise the curve stays where it is and lambda <- min(lambda ``up``, 1e8).  The energy is
    therefore monotone non-increasing, and ``steps=0`` gives the diagnostics of the straight latent line."""

    def __init__(self, density, points=17, steps=10, damping=1e-3, up=10.0, down=0.1):
        self.density, self.head = density, metric_head(density, "latent", "manifold geodesics")
        d = self.head.program.d
        if d > E.GEODESIC_MAX_WIDTH:
            raise ValueError(f"latent_dimension = {d}: manifold geodesics support 1 <= latent_dimension <= "
                             f"{E.GEODESIC_MAX_WIDTH} (DESIGN 9)")
        if int(points) < 3 or int(steps) < 0 or not damping >= 0 or not up >= 1 or not 0 < down <= 1:
            raise ValueError(f"need points >= 3, steps >= 0, damping >= 0, up >= 1 and 0 < down <= 1, got {points}, {steps}, "
                             f"{damping}, {up}, {down}")
        self.points, self.steps = int(points), int(steps)
        self.damping, self.up, self.down = float(damping), float(up), float(down)
        # the encoder's latent under the head's one-shot pre-hook and the bijections in front of the head: the projector's
        self.projector = ManifoldProjector(density, steps=0)
        self.chain = self.projector.chain

    def evaluate(self, z, lam):
        """Decode with tangents at the curve-major latents ``z`` (B, P, d), Gram, cross-Gram, curve step kernel: the
        ``engine.CurveStepResult``."""
        prog, P = self.head.program, self.points
        x_hat, T = prog.decode(z.reshape(-1, prog.d), tangents=True)
        jtj = E.gram_cholesky(T, prog.d, 1).jtj
        cross = E.cross_gram(T, prog.d, P)
        return E.curve_step(T, jtj, cross, x_hat.contiguous(), P, lam)

    @torch.no_grad()
    def connect(self, x0, x1, steps=None):
        """The curves between the inputs ``x0`` and ``x1`` (the density's inputs, (B, *x_shape) each, as for ``elbo`` / ``ood``;
        never modified, no dequantisation noise is drawn): ``connect_latents`` between the encoder's latents."""
        E.require_gpu(x0, "x0")
        E.require_gpu(x1, "x1")
        if x0.shape != x1.shape or x0.device != x1.device:
            raise ValueError(f"x0 {tuple(x0.shape)} on {x0.device} and x1 {tuple(x1.shape)} on {x1.device} must agree")
        if x0.shape[0] == 0:
            raise ValueError("connect needs at least one pair of inputs")
        with E.scope(self.head.kernels):
            z0 = self.projector.head_input_and_latent(x0)[1]
            z1 = self.projector.head_input_and_latent(x1)[1]
        return self.connect_latents(z0, z1, steps)

    @torch.no_grad()
    def connect_latents(self, z0, z1, steps=None):
        """Relax the curves between the head's latents ``z0`` and ``z1`` ((B, d) float32 each).  Returns device tensors for the B
        curves of P points, N = P - 1 segments and M = P - 2 interior points:
          ``latents`` (B, P, d) float32; ``path_head`` (B, P, *x_shape) = g(latents) in the head's input space and ``path``, the same
          mapped back to data space; ``energy`` and ``initial_energy`` (B,) float64, E = N sum_i ||r_i||^2 of the returned curve and
          of the straight latent line; ``length`` and ``initial_length`` (B,) float64, L = sum_i ||r_i|| (L^2 <= E, equal at constant
          speed); ``segment_lengths`` (B, N) float64; ``gradient`` (B, M, d) float64 = J_i^T (x_{i-1} + x_{i+1} - 2 x_i) at the
          returned curve and ``gradient_max`` (B,) its largest magnitude; ``accepted`` (B,) int32, the steps taken; ``damping``
          (B,) float64, the final lambda; ``info`` (B,) int32, the code of the closing evaluation (``engine.curve_step``).
        Sub-batches of whole curves like the log-density path; enqueues kernels only -- no copy to the host, no synchronisation --
        and leaves ``head.last_gram`` alone."""
        E.require_gpu(z0, "z0")
        E.require_gpu(z1, "z1")
        steps = self.steps if steps is None else int(steps)
        prog, P = self.head.program, self.points
        if z0.dim() != 2 or z0.shape[1] != prog.d or z0.shape != z1.shape or z0.device != z1.device:
            raise ValueError(f"z0 {tuple(z0.shape)} on {z0.device} and z1 {tuple(z1.shape)} on {z1.device} must both be (B, {prog.d})")
        B = z0.shape[0]
        if B == 0 or steps < 0:
            raise ValueError(f"connect needs at least one curve and steps >= 0, got {B} curves and steps = {steps}")
        chunk = prog.tangent_chunk(B * P) // P
        if chunk == 0:
            raise ValueError(f"points = {P}: one curve of {P} points does not fit the sub-batch of {prog.tangent_chunk(B * P)} "
                             f"samples a decode sweep may hold; use fewer points")
        with E.scope(self.head.kernels):
            parts = [self._connect(z0[i:i + chunk], z1[i:i + chunk], steps) for i in range(0, B, chunk)]
        return parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts]) for k in parts[0]}

    def _connect(self, z0, z1, steps):
        prog, B, dev, P = self.head.program, z0.shape[0], z0.device, self.points
        N, d = P - 1, prog.d
        tt = torch.arange(P, dtype=torch.float32, device=dev) / N
        z = z0[:, None, :] + tt[None, :, None] * (z1 - z0)[:, None, :]          # the straight latent line
        z[:, N] = z1
        decode = lambda zz: prog.decode(zz.reshape(-1, d), tangents=False)[0].contiguous()
        x_hat = decode(z)
        seg2, total, _ = E.curve_energy(x_hat, P)
        energy = total * N
        seg2_0, energy_0 = seg2.clone(), energy.clone()
        lam = torch.full((B,), self.damping, dtype=torch.float64, device=dev)
        accepted = torch.zeros(B, dtype=torch.int32, device=dev)
        wide = (B,) + (1,) * (x_hat.dim())                                      # over (B, P, *x_shape)
        curves = lambda x: x.view(B, P, *x.shape[1:])
        for _ in range(steps):
            r = self.evaluate(z, lam)
            solved = r.info == 0
            z_new = z.clone()
            z_new[:, 1:N] += torch.where(solved[:, None, None], r.delta, torch.zeros_like(r.delta)).float()
            x_new = decode(z_new)
            seg2_new, total_new, _ = E.curve_energy(x_new, P)
            energy_new = total_new * N
            ok = solved & (energy_new < energy)                                 # a NaN energy compares false: rejected
            z = torch.where(ok[:, None, None], z_new, z)
            x_hat = torch.where(ok.view(wide), curves(x_new), curves(x_hat)).view_as(x_hat)
            seg2 = torch.where(ok[:, None], seg2_new, seg2)
            energy = torch.where(ok, energy_new, energy)
            lam = torch.where(ok, (lam * self.down).clamp_min(DAMPING_MIN), (lam * self.up).clamp_max(DAMPING_MAX))
            accepted += ok
        r = self.evaluate(z, torch.zeros_like(lam))
        x_data = x_hat
        for bijection in reversed(self.chain):
            x_data = bijection.z_to_x(x_data)["x"]
        lengths, lengths_0 = seg2.sqrt(), seg2_0.sqrt()
        return {"latents": z, "path_head": curves(x_hat), "path": curves(x_data), "energy": energy, "initial_energy": energy_0,
                "length": lengths.sum(1), "initial_length": lengths_0.sum(1), "segment_lengths": lengths, "gradient": r.grad,
                "gradient_max": r.stats[:, 3].contiguous(), "accepted": accepted, "damping": lam, "info": r.info}
