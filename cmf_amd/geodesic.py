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

``connect`` is the logarithm side; ``shoot`` is the exponential map: from a point and a latent velocity it walks along
the manifold's own geodesic by classical RK4 on Hamilton's equations z' = G^-1 p, p' = grad_z 1/2 ||J(z) v||^2 (v held fixed), so no
second derivative of the decoder is formed.  One evaluation is a primal decode that keeps state, a d-column sweep for G, the
per-sample float64 solve (csrc/shoot_step.hip), a one-direction sweep that is kept, and the training backward.

    lg = geo.log(x0, x1)                                 # connect + the initial velocity of the relaxed curve
    out = geo.shoot(x0, lg["velocity"])                  # out["path"][:, -1] is close to x1
    out = geo.shoot_latents(z0, v0, steps=8, time=0.5)

``transport`` is parallel transport: a latent tangent direction at one input carried along the geodesic to another,
keeping its length and its angles in the pull-back metric.  Per segment it averages the projection onto the next tangent plane
with the inverse of the projection back (csrc/transport_step.hip, float64 per curve), which is second order in the segment.

    tr = geo.transport(x0, x1, w)                        # connect + w (B, d) or (B, d, m) at x0 carried to x1
    tr["transported"], tr["norm2"]                       # (B, d, m) at x1; w^T G w at every point of the curve
    out = geo.analogy(xa, xb, xc)                        # "a is to b as c is to ?": out["path"][:, -1]

``mean`` takes more than two inputs: the Frechet (Karcher) mean of K inputs, their weighted barycentre on the
manifold.  It relaxes the whole star -- K discretised arms that share one free end point -- at once; a step is one decode sweep over
the stars and a float64 solve of the block-arrow normal equations, arm by arm with only the centre block shared
(csrc/star_step.hip).

    out = geo.mean(xs, weights)                          # xs (B, K, *x_shape): out["mean"] (B, *x_shape) in data space
    out["distances"], out["variance"]                    # (B, K) arm lengths; the estimate of the Frechet variance

``principal`` is the step after the mean: principal geodesic analysis, PCA in the tangent plane at the Frechet mean in
the pull-back metric.  The arms of the relaxed star give the log vector of every input at the mean, one decode sweep gives G there,
and one float64 kernel per group (csrc/tangent_pca.hip) diagonalises the weighted covariance in its dual K x K form.

    pga = geo.principal(xs, weights)                     # the values of mean, and beside them
    pga["variances"], pga["explained"], pga["rank"]      # (B, r) variance per mode and its share; the numerical rank
    pga["directions"], pga["scores"]                     # (B, r, d) G-orthonormal modes; (B, K, r) coordinates of the inputs
    walk = geo.principal_paths(pga, component=0)         # walk["path"]: -2 .. +2 standard deviations along the first mode
"""
import math
import numbers

import torch

from . import engine as E
from .metric_stats import metric_head
from .projection import ManifoldProjector, join_parts, lm_loop, to_data_space

__all__ = ["ManifoldGeodesic"]


class ManifoldGeodesic:
    """Damped Gauss-Newton relaxation of discretised curves on the manifold of a non-square density with latent dimension <= 128.

    A curve has ``points`` >= 3 latents; its ends stay where they are.  ``steps`` iterations per call; every curve carries its own
    damping lambda, started at ``damping``: a step is accepted iff its solve succeeded and it strictly lowers the energy, then
    lambda <- max(lambda ``down``, 1e-12); otherwise the curve stays where it is and lambda <- min(lambda ``up``, 1e8).  The energy is
    therefore monotone non-increasing, and ``steps=0`` gives the diagnostics of the straight latent line.

    ``shoot`` / ``shoot_latents`` integrate the geodesic that leaves a point with a given latent velocity in ``shoot_steps`` >= 1
    RK4 steps (``log`` / ``log_latents``: ``connect`` plus the velocity that takes ``shoot`` from the first end to the second).

    ``transport`` / ``transport_latents`` carry latent tangent vectors along a curve by parallel transport; ``analogy`` carries the
    ``log`` velocity of one pair of inputs to a third input and shoots along it there.

    ``mean`` / ``mean_latents`` find the weighted Frechet mean of K inputs: the loop above with a star of K arms of ``points``
    latents and one shared free end point as its unit.

    ``principal`` / ``principal_latents`` add the principal modes of variation of the K inputs around that mean (principal geodesic
    analysis); ``principal_paths`` draws a mode by shooting from the mean in both directions."""

    def __init__(self, density, points=17, steps=10, damping=1e-3, up=10.0, down=0.1, shoot_steps=16):
        if int(shoot_steps) < 1:
            raise ValueError(f"need shoot_steps >= 1, got {shoot_steps}")
        self.shoot_steps = int(shoot_steps)
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
        return join_parts(parts)

    def _connect(self, z0, z1, steps):
        prog, B, dev, P = self.head.program, z0.shape[0], z0.device, self.points
        N, d = P - 1, prog.d
        tt = torch.arange(P, dtype=torch.float32, device=dev) / N
        z = z0[:, None, :] + tt[None, :, None] * (z1 - z0)[:, None, :]          # the straight latent line
        z[:, N] = z1
        curves = lambda x: x.view(B, P, *x.shape[1:])

        def at(z):                                              # the state of ``lm_loop``: (z, g(z) as (B, P, *x_shape), ||r_i||^2, E)
            x_hat = prog.decode(z.reshape(-1, d), tangents=False)[0].contiguous()
            seg2, total, _ = E.curve_energy(x_hat, P)
            return z, curves(x_hat), seg2, total * N

        def trial(state, lam):
            r = self.evaluate(state[0], lam)
            solved = r.info == 0
            z_new = state[0].clone()
            z_new[:, 1:N] += torch.where(solved[:, None, None], r.delta, torch.zeros_like(r.delta)).float()
            return solved, at(z_new)

        state = at(z)
        seg2_0, energy_0 = state[2].clone(), state[3].clone()
        lam = torch.full((B,), self.damping, dtype=torch.float64, device=dev)
        (z, x_hat, seg2, energy), lam, accepted = lm_loop(state, 3, lam, steps, self.up, self.down, trial)
        r = self.evaluate(z, torch.zeros_like(lam))
        x_data = to_data_space(self.chain, x_hat.flatten(0, 1))
        lengths, lengths_0 = seg2.sqrt(), seg2_0.sqrt()
        return {"latents": z, "path_head": x_hat, "path": curves(x_data), "energy": energy, "initial_energy": energy_0,
                "length": lengths.sum(1), "initial_length": lengths_0.sum(1), "segment_lengths": lengths, "gradient": r.grad,
                "gradient_max": r.stats[:, 3].contiguous(), "accepted": accepted, "damping": lam, "info": r.info}

    # -- Frechet means ---------------------------------------------------------------------------
    def evaluate_star(self, z, weights, lam):
        """Decode with tangents at the stars ``z`` (B, K, P, d) -- one sweep over the star-major stack --, Gram, the cross-Gram blocks
        of its neighbouring samples (``engine.star_cross_gram``: no padding samples in the sweep), star step kernels: the
        ``engine.StarStepResult``."""
        prog = self.head.program
        B, K, P, d = z.shape
        x_hat, T = prog.decode(z.reshape(B * K * P, d), tangents=True)
        jtj = E.gram_cholesky(T, d, 1).jtj
        return E.star_step(T, jtj, E.star_cross_gram(T, d), x_hat.contiguous(), P, K, weights, lam)

    @torch.no_grad()
    def mean(self, xs, weights=None, steps=None):
        """The Frechet (Karcher) mean of the K inputs ``xs[b]`` for every b (``xs``: (B, K, *x_shape), the density's inputs as for
        ``connect``; never modified, no dequantisation noise is drawn): ``mean_latents`` of the encoder's latents."""
        if not isinstance(xs, torch.Tensor) or xs.dim() < 3:
            raise ValueError(f"xs must be (B, K, *x_shape), got {tuple(getattr(xs, 'shape', ()))}")
        if xs.shape[0] == 0 or xs.shape[1] == 0:
            raise ValueError(f"mean needs at least one group of at least one input, got xs {tuple(xs.shape)}")
        E.require_gpu(xs, "xs")
        with E.scope(self.head.kernels):
            z = self.projector.head_input_and_latent(xs.flatten(0, 1))[1]
        return self.mean_latents(z.view(xs.shape[0], xs.shape[1], -1), weights, steps)

    @staticmethod
    def _star_weights(weights, B, K):
        """``weights`` as given ((B, K) or (K,), floating point, finite and > 0; None: all ones) or a ValueError.  The values are
        looked at where they are: weights on the device make the call wait for them once."""
        if weights is None:
            return None
        if not isinstance(weights, torch.Tensor) or not weights.is_floating_point() or tuple(weights.shape) not in ((B, K), (K,)):
            raise ValueError(f"weights must be a floating point tensor of shape ({B}, {K}) or ({K},), got "
                             f"{tuple(getattr(weights, 'shape', ()))} {getattr(weights, 'dtype', type(weights).__name__)}")
        if not bool((torch.isfinite(weights) & (weights > 0)).all()):
            raise ValueError("weights must be finite and > 0")
        return weights

    @torch.no_grad()
    def mean_latents(self, zs, weights=None, steps=None):
        """The weighted Frechet mean of the head's latents ``zs`` (B, K, d) float32 per group b: the point m that minimises
        sum_k w_k dist(m, z_k)^2 in the pull-back metric, found by relaxing the whole star at once -- K discretised arms of P =
        ``points`` latents from the inputs to one shared free end point, the centre --, E = sum_k w_k N sum_i ||r_{k,i}||^2 over all
        interior points and the centre by the damped Gauss-Newton loop of ``connect`` with the star as unit.  ``weights``: (B, K) or
        (K,), floating point, finite and > 0, used as given (not normalised); default all ones.  The start is the centre at
        sum_k w_k z_k / sum_k w_k with every arm on the straight latent line.  Returns device tensors for the B stars of K arms with
        N = P - 1 segments and M = P - 2 interior points each:
          ``mean_latent`` (B, d) float32; ``mean_head`` (B, *x_shape) = g(mean_latent) in the head's input space and ``mean``, the
          same mapped back to data space; ``latents`` (B, K, P, d) float32 (``[:, k, 0]`` = z_k, ``[:, k, -1]`` = mean_latent);
          ``path_head`` and ``path`` (B, K, P, ...); ``distances`` and ``initial_distances`` (B, K) float64, the arm lengths sum_i
          ||r_{k,i}|| of the returned star and of the start; ``segment_lengths`` (B, K, N) float64; ``energy`` and
          ``initial_energy`` (B,) float64; ``variance`` (B,) float64 = energy / sum_k w_k, the estimate of the Frechet variance;
          ``gradient`` (B, K, M, d) and ``gradient_centre`` (B, d) float64 at the returned star and ``gradient_max`` (B,) their
          largest magnitude; ``accepted`` (B,) int32; ``damping`` (B,) float64; ``info`` (B,) int32, the code of the closing
          evaluation (``engine.star_step``).
        Sub-batches of whole stars; enqueues kernels only -- beyond the look at ``weights`` no copy to the
        host, no synchronisation -- and leaves ``head.last_gram`` alone."""
        return self._relax_stars(zs, *self._star_arguments(zs, weights, steps))[0]

    def _star_arguments(self, zs, weights, steps):
        """The refusals of ``mean_latents`` that need no GPU: (steps, weights as ``_star_weights`` gives them) or a ValueError."""
        prog = self.head.program
        if not isinstance(zs, torch.Tensor) or zs.dim() != 3 or zs.shape[2] != prog.d or zs.dtype != torch.float32:
            raise ValueError(f"zs must be (B, K, {prog.d}) float32, got {tuple(getattr(zs, 'shape', ()))} "
                             f"{getattr(zs, 'dtype', type(zs).__name__)}")
        B, K = zs.shape[0], zs.shape[1]
        steps = self.steps if steps is None else int(steps)
        if B == 0 or steps < 0 or not 1 <= K <= E.STAR_MAX_ARMS:
            raise ValueError(f"mean needs at least one group of 1 <= K <= {E.STAR_MAX_ARMS} inputs and steps >= 0, got {B} groups "
                             f"of {K} and steps = {steps}")
        return steps, self._star_weights(weights, B, K)

    def _relax_stars(self, zs, steps, weights):
        """``mean_latents`` behind its refusals: (its values, the weights as the kernels saw them: (B, K) float64)."""
        prog, P = self.head.program, self.points
        B, K = zs.shape[0], zs.shape[1]
        E.require_gpu(zs, "zs")
        dev = zs.device
        if weights is None:
            w = torch.ones(B, K, dtype=torch.float64, device=dev)
        else:
            w = weights.to(device=dev, dtype=torch.float64).expand(B, K).contiguous()
        chunk = prog.tangent_chunk(B * K * P) // (K * P)
        if chunk == 0:
            raise ValueError(f"points = {P}: one star of {K} inputs with {P} points per arm does not fit the sub-batch of "
                             f"{prog.tangent_chunk(B * K * P)} samples a decode sweep may hold; use fewer points or fewer inputs")
        with E.scope(self.head.kernels):
            parts = [self._mean(zs[i:i + chunk], w[i:i + chunk].contiguous(), steps) for i in range(0, B, chunk)]
        return join_parts(parts), w

    def _mean(self, zs, w, steps):
        prog, dev, P = self.head.program, zs.device, self.points
        B, K, d = zs.shape
        N = P - 1
        arm_sum = lambda t: sum((w[:, k] * t[:, k] for k in range(1, K)), w[:, 0] * t[:, 0])      # (B, K) -> (B,), in arm order
        w_sum = arm_sum(torch.ones_like(w))
        zc = (sum((w[:, k, None] * zs[:, k].double() for k in range(1, K)), w[:, 0, None] * zs[:, 0].double()) / w_sum[:, None]).float()
        tt = torch.arange(P, dtype=torch.float32, device=dev) / N
        z = zs[:, :, None, :] + tt[None, None, :, None] * (zc[:, None, :] - zs)[:, :, None, :]       # straight latent arms
        z[:, :, N] = zc[:, None, :]
        stars = lambda x: x.view(B, K, P, *x.shape[1:])

        def at(z):                                              # the state of ``lm_loop``: (z, g(z), ||r_{k,i}||^2, E)
            x_hat = prog.decode(z.reshape(-1, d), tangents=False)[0].contiguous()
            seg2, total, _ = E.curve_energy(x_hat, P)
            return z, stars(x_hat), seg2.view(B, K, N), arm_sum(total.view(B, K)) * N

        def trial(state, lam):
            r = self.evaluate_star(state[0], w, lam)
            solved = r.info == 0
            z_new = state[0].clone()
            z_new[:, :, 1:N] += torch.where(solved[:, None, None, None], r.delta, torch.zeros_like(r.delta)).float()
            z_new[:, :, N] += torch.where(solved[:, None], r.delta_centre, torch.zeros_like(r.delta_centre)).float()[:, None, :]
            return solved, at(z_new)

        state = at(z)
        seg2_0, energy_0 = state[2].clone(), state[3].clone()
        lam = torch.full((B,), self.damping, dtype=torch.float64, device=dev)
        (z, x_hat, seg2, energy), lam, accepted = lm_loop(state, 3, lam, steps, self.up, self.down, trial)
        r = self.evaluate_star(z, w, torch.zeros_like(lam))
        x_data = to_data_space(self.chain, x_hat.flatten(0, 2))
        lengths, lengths_0 = seg2.sqrt(), seg2_0.sqrt()
        path = stars(x_data)
        return {"mean_latent": z[:, 0, N].contiguous(), "mean_head": x_hat[:, 0, N].contiguous(), "mean": path[:, 0, N].contiguous(),
                "latents": z, "path_head": x_hat, "path": path, "distances": lengths.sum(2),
                "initial_distances": lengths_0.sum(2), "segment_lengths": lengths, "energy": energy, "initial_energy": energy_0,
                "variance": energy / w_sum, "gradient": r.grad, "gradient_centre": r.grad_centre,
                "gradient_max": r.stats[:, 3].contiguous(), "accepted": accepted, "damping": lam, "info": r.info}

    # -- principal geodesic analysis --------------------------------------------------------------
    @torch.no_grad()
    def principal(self, xs, weights=None, components=None, steps=None):
        """Principal geodesic analysis of the K inputs ``xs[b]`` for every b (``xs``, ``weights``, ``steps`` as for ``mean``):
        ``principal_latents`` of the encoder's latents."""
        if not isinstance(xs, torch.Tensor) or xs.dim() < 3:
            raise ValueError(f"xs must be (B, K, *x_shape), got {tuple(getattr(xs, 'shape', ()))}")
        if xs.shape[0] == 0 or xs.shape[1] == 0:
            raise ValueError(f"principal needs at least one group of at least one input, got xs {tuple(xs.shape)}")
        E.require_gpu(xs, "xs")
        with E.scope(self.head.kernels):
            z = self.projector.head_input_and_latent(xs.flatten(0, 1))[1]
        return self.principal_latents(z.view(xs.shape[0], xs.shape[1], -1), weights, components, steps)

    @torch.no_grad()
    def principal_latents(self, zs, weights=None, components=None, steps=None):
        """The principal modes of variation of the head's latents ``zs`` (B, K, d) float32 per group b: PCA in the tangent plane at
        their Frechet mean in the pull-back metric G = J^T J.  ``mean_latents(zs, weights, steps)`` finds the mean; the log vector of
        input k there is the end difference v_k = N (-3 z_{k,N} + 4 z_{k,N-1} - z_{k,N-2}) / 2 of arm k of the relaxed star, in
        float64 (it points from the mean towards input k and reaches it in time 1: the mirror image of ``log``'s velocity); G comes
        from one decode sweep with tangents over the B centres; one kernel (csrc/tangent_pca.hip) diagonalises the weighted
        covariance sum_k w_k v_k v_k^T G / sum_k w_k in its dual K x K form.  ``components`` = r modes are returned: None means
        min(K, d), else 1 <= components <= min(K, d).  Returns the values of ``mean_latents``, unchanged, and beside them:
          ``log_velocities`` (B, K, d) float64; ``metric`` (B, d, d) float32, G at the mean exactly as the kernel read it (its lower
          triangle); ``variances`` (B, r) float64, descending: the variance along mode j in squared geodesic length;
          ``directions`` (B, r, d) float64, the modes u_j as latent components, G-orthonormal, largest-magnitude component positive;
          ``scores`` (B, K, r) float64 = u_j^T G v_k, the coordinate of input k along mode j; ``covectors`` (B, K, d) float64 =
          G v_k; ``norm2`` (B, K) float64 = v_k^T G v_k, the squared geodesic distance the log vector of arm k claims (compare
          ``distances``); ``total_variance`` (B,) float64 = sum_k w_k norm2_k / sum_k w_k; ``explained`` (B, r) float64 =
          variances / total_variance, 0 where that is 0; ``rank`` (B,) int32, the modes whose variance is above d 2^-24 times the
          largest -- below that a float32 metric leaves it undetermined --: the others have zero directions and scores; ``pga_info``
          (B,) int32, the code of ``engine.tangent_pca`` (``info`` stays ``mean_latents``').
        K copies of one input give rank 0 and exact zeros.  Enqueues kernels only -- beyond ``mean_latents``' look at ``weights`` no
        copy to the host, no synchronisation -- and leaves ``head.last_gram`` alone."""
        steps, weights = self._star_arguments(zs, weights, steps)
        prog, N = self.head.program, self.points - 1
        B, K, d = zs.shape
        most = min(K, d)
        r = most if components is None else components
        if isinstance(r, bool) or not isinstance(r, numbers.Integral) or not 1 <= r <= most:
            raise ValueError(f"components = {components!r}: need None or an integer 1 <= components <= min(K, d) = {most}")
        out, w = self._relax_stars(zs, steps, weights)
        out = dict(out)
        z = out["latents"].double()
        logv = ((self.points - 1) * (-3.0 * z[:, :, N] + 4.0 * z[:, :, N - 1] - z[:, :, N - 2]) / 2.0).contiguous()
        centre = out["mean_latent"]
        chunk = prog.tangent_chunk(B)
        with E.scope(self.head.kernels):
            parts = []
            for i in range(0, B, chunk):
                _, T = prog.decode(centre[i:i + chunk], tangents=True)
                parts.append(E.gram_cholesky(T, d, 1).jtj)
                del T
            metric = (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous()
            pca = E.tangent_pca(metric, logv, w, r)
        positive = pca.total > 0
        explained = torch.where(positive[:, None], pca.variances / torch.where(positive, pca.total, torch.ones_like(pca.total))[:, None],
                                torch.zeros_like(pca.variances))
        out.update(log_velocities=logv, metric=metric, variances=pca.variances, directions=pca.directions, scores=pca.scores,
                   covectors=pca.covectors, norm2=pca.norm2, total_variance=pca.total, explained=explained, rank=pca.rank,
                   pga_info=pca.info)
        return out

    @torch.no_grad()
    def principal_paths(self, result, component=0, extent=2.0, steps=None):
        """Draw mode ``component`` of a ``principal`` / ``principal_latents`` result: the geodesics that leave the mean with the
        latent velocities -/+ ``extent`` sqrt(lambda_j) u_j, ``extent`` standard deviations along the mode in each direction, by one
        ``shoot_latents`` call of 2 B trajectories of S = ``steps`` (default ``shoot_steps``) steps.  Returns device tensors:
          ``path``, ``path_head`` and ``latents`` (B, 2 S + 1, ...): the two halves joined through the mean, running from -extent
          (node 0) through the mean (node S) to +extent (node 2 S); ``speed2`` (B, 2, S + 1) and ``info`` (B, 2) of ``shoot_latents``,
          [:, 0] the negative half and [:, 1] the positive one, each from the mean outwards.
        A group whose rank is <= ``component`` has zero velocity and stays at the mean."""
        need = ("mean_latent", "mean_head", "mean", "variances", "directions")
        if not isinstance(result, dict) or any(key not in result for key in need):
            raise ValueError("result must be what principal / principal_latents returned")
        lam, u, z0 = result["variances"], result["directions"], result["mean_latent"]
        j, extent = int(component), float(extent)
        if not 0 <= j < lam.shape[1]:
            raise ValueError(f"component = {component}: the result holds the components 0 .. {lam.shape[1] - 1}")
        if not (math.isfinite(extent) and extent > 0):
            raise ValueError(f"principal_paths needs a finite extent > 0, got {extent}")
        B = z0.shape[0]
        v = (extent * lam[:, j].clamp_min(0.0).sqrt())[:, None] * u[:, j]                  # zero beyond the rank: u_j is
        shot = self.shoot_latents(torch.cat([z0, z0]), torch.cat([-v, v]), steps)
        S = shot["latents"].shape[1] - 1
        halves = lambda t: t.view(2, B, *t.shape[1:])
        # the middle node is the result's own mean (the shot's node 0 decodes the same latent on another path)
        join = lambda t, mean: torch.cat([halves(t)[0][:, 1:].flip(1), mean[:, None], halves(t)[1][:, 1:]], 1)
        return {"path": join(shot["path"], result["mean"]), "path_head": join(shot["path_head"], result["mean_head"]),
                "latents": join(shot["latents"], z0),
                "speed2": halves(shot["speed2"]).transpose(0, 1).contiguous(), "info": halves(shot["info"]).transpose(0, 1).contiguous()}

    # -- the exponential map -----------------------------------------------------------------
    @torch.no_grad()
    def log(self, x0, x1, steps=None):
        """``connect(x0, x1, steps)`` and, beside its values, ``velocity`` (B, d) float64: the latent velocity of the relaxed curve at
        its start, the second-order one-sided difference N (-3 z_0 + 4 z_1 - z_2) / 2 of its ``latents`` -- what ``shoot`` takes to
        walk from ``x0`` to ``x1`` in time 1."""
        return self._with_velocity(self.connect(x0, x1, steps))

    @torch.no_grad()
    def log_latents(self, z0, z1, steps=None):
        """``connect_latents(z0, z1, steps)`` with the ``velocity`` of ``log``."""
        return self._with_velocity(self.connect_latents(z0, z1, steps))

    def _with_velocity(self, out):
        z = out["latents"].double()
        out = dict(out)
        out["velocity"] = (self.points - 1) * (-3.0 * z[:, 0] + 4.0 * z[:, 1] - z[:, 2]) / 2.0
        return out

    def _metric(self, z32):
        """One primal decode at ``z32`` that keeps state and the unsaved d-column sweep over it: (x_hat, primal contexts, jtj)."""
        prog = self.head.program
        x_hat, _, pctx = prog.decode_train(z32, tangents=False, nc_hint=16)
        T, _ = prog.decode_tangents_from_ctx(pctx)
        jtj = E.gram_cholesky(T, prog.d, 1).jtj
        del T
        return x_hat, pctx, jtj

    @torch.no_grad()
    def shoot_evaluate(self, z, p, grads, backward=True, metric=None):
        """The right-hand side of Hamilton's equations at the latents ``z`` (B, d) float32 and momenta ``p`` (B, d) float64:
        returns (p' (B, d) float64, v = G^-1 p (B, d) float64, p^T v (B,) float64, info (B,) int32, x_hat).  ``info``: the code of
        ``engine.metric_solve`` (0 ok; 1 a non-positive pivot of G, 2 a non-finite value: v, p' and the speed are NaN).  ``grads``: an
        ``engine.GradPool`` over the head's parameters that the backward fills and nobody reads.  ``backward=False``
        stops after the solve (p' is None); ``metric``: the result of ``_metric(z)`` where the caller has it already."""
        prog = self.head.program
        with E.scope(self.head.kernels):
            x_hat, pctx, jtj = self._metric(z) if metric is None else metric
            r = E.metric_solve(jtj, p)
            speed2 = r.stats[:, 0].contiguous()
            if not backward:
                return None, r.out64, speed2, r.info, x_hat
            TV, ctx = prog.decode_tangents_from_ctx(pctx, eps=r.out32[:, :, None], nc=16, save=True)
            # 1/2 ||J v||^2 of the one direction v: its cotangent on the stack is J v itself, in place in a copy
            Ct = E.Tangent(TV.B, TV.N, TV.nc, TV.layout, TV.data.device, data=TV.data.clone(), compact=TV.compact)
            dz = prog.decode_backward(ctx, Ct, torch.zeros_like(x_hat), grads)
        return dz.double(), r.out64, speed2, r.info, x_hat

    @torch.no_grad()
    def shoot(self, x, v0, steps=None, time=1.0):
        """The geodesic that leaves the input ``x`` (the density's input, (B, *x_shape), as for ``connect``; never modified) with the
        latent velocity ``v0`` (B, d): ``shoot_latents`` from the encoder's latent."""
        E.require_gpu(x, "x")
        if x.shape[0] == 0:
            raise ValueError("shoot needs at least one input")
        with E.scope(self.head.kernels):
            z0 = self.projector.head_input_and_latent(x)[1]
        return self.shoot_latents(z0, v0, steps, time)

    @torch.no_grad()
    def shoot_latents(self, z0, v0, steps=None, time=1.0):
        """Walk from the head's latents ``z0`` (B, d) float32 with the latent velocities ``v0`` (B, d) (float64, or float32) for
        ``time`` along the geodesics of the pull-back metric G = J^T J: classical RK4 with ``steps`` (default ``shoot_steps``) equal
        steps on z' = G^-1 p, p' = grad_z 1/2 ||J(z) v||^2, from p_0 = G(z_0) v_0.  z and p are carried in float64; the decoder sees
        ``z.float()``.  Returns device tensors for the B trajectories of S + 1 nodes:
          ``latents`` (B, S + 1, d) float32; ``velocity`` and ``momentum`` (B, S + 1, d) float64; ``speed2`` (B, S + 1) float64 =
          p^T v = ||d gamma / dt||^2 at every node; ``length`` (B,) float64, the trapezoid of sqrt(speed2) over the steps taken;
          ``path_head`` (B, S + 1, *x_shape) = g(latents) in the head's input space and ``path``, the same mapped back to data space;
          ``steps_taken`` (B,) int32; ``info`` (B,) int32, 0 or the first failure code of ``engine.metric_solve``.
        A trajectory one of whose evaluations fails is frozen at its last good node: its later nodes repeat that node, the other
        trajectories are unaffected.

        p^T v is conserved wherever G is differentiable, and on tanh-MLP couplers RK4 shows clean fourth order.  ResNet couplers are
        piecewise linear: J, G and the Hamiltonian jump across ReLU boundaries while an explicit integrator keeps p continuous, so
        ``speed2`` shows jumps of up to a few per cent that do NOT shrink with the step; ``speed2`` is the record to
        read.  Sub-batches like a training step; enqueues kernels only -- no copy to the host, no synchronisation -- and leaves
        ``head.last_gram`` and ``head.last_hutchinson`` alone."""
        E.require_gpu(z0, "z0")
        steps = self.shoot_steps if steps is None else int(steps)
        prog = self.head.program
        if z0.dim() != 2 or z0.shape[1] != prog.d or not isinstance(v0, torch.Tensor) or v0.shape != z0.shape or \
                v0.device != z0.device or not v0.is_floating_point():
            raise ValueError(f"z0 {tuple(z0.shape)} on {z0.device} and v0 {tuple(getattr(v0, 'shape', ()))} on "
                             f"{getattr(v0, 'device', type(v0).__name__)} must both be (B, {prog.d})")
        B = z0.shape[0]
        if B == 0 or steps < 1:
            raise ValueError(f"shoot needs at least one trajectory and steps >= 1, got {B} trajectories and steps = {steps}")
        time = float(time)
        if not (math.isfinite(time) and time > 0):
            raise ValueError(f"shoot needs a finite time > 0, got {time}")
        dev = z0.device
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        chunk = max(1, min(prog.tangent_chunk(B), int(0.8 * free // max(prog.train_bytes_per_sample(16), 1))))
        grads = E.GradPool([q for q in self.head.parameters() if q.requires_grad], dev)
        v0 = v0.double().contiguous()
        with E.scope(self.head.kernels):
            parts = [self._shoot(z0[i:i + chunk].contiguous(), v0[i:i + chunk], steps, time, grads) for i in range(0, B, chunk)]
        return join_parts(parts)

    def _shoot(self, z0, v0, steps, time, grads):
        B, dev, h = z0.shape[0], z0.device, time / steps
        z = z0.double()
        first = self._metric(z0)
        mom = E.metric_solve(first[2], v0, apply=True)                          # p_0 = G(z_0) v_0
        p = mom.out64
        dp, v, s2, info, x_hat = self.shoot_evaluate(z0, p, grads, metric=first)
        del first
        alive = info == 0
        taken = torch.zeros(B, dtype=torch.int32, device=dev)
        wide = (B,) + (1,) * (x_hat.dim() - 1)
        nodes = [(z.float(), v, p, s2, x_hat)]
        for i in range(steps):
            # the node's own evaluation is the first stage; three more, then the evaluation of the new node
            codes, kz, kp = [], [v], [dp]
            for a in (0.5, 0.5, 1.0):
                dpa, va, _, ia, _ = self.shoot_evaluate((z + (a * h) * kz[-1]).float(), p + (a * h) * kp[-1], grads)
                kz.append(va)
                kp.append(dpa)
                codes.append(ia)
            z_new = z + (h / 6.0) * (kz[0] + 2.0 * kz[1] + 2.0 * kz[2] + kz[3])
            p_new = p + (h / 6.0) * (kp[0] + 2.0 * kp[1] + 2.0 * kp[2] + kp[3])
            # the closing evaluation gives the speed at the last node and needs no backward
            dp_new, v_new, s2_new, i_new, x_new = self.shoot_evaluate(z_new.float(), p_new, grads, backward=i + 1 < steps)
            codes.append(i_new)
            code = codes[3]
            for c in reversed(codes[:3]):                                       # the first failure code of the step
                code = torch.where(c != 0, c, code)
            ok = alive & (code == 0)
            info = torch.where(alive & ~ok, code, info)
            z, p = torch.where(ok[:, None], z_new, z), torch.where(ok[:, None], p_new, p)
            v, s2 = torch.where(ok[:, None], v_new, v), torch.where(ok, s2_new, s2)
            if dp_new is not None:
                dp = torch.where(ok[:, None], dp_new, dp)
            x_hat = torch.where(ok.view(wide), x_new, x_hat)
            alive = ok
            taken += ok
            nodes.append((z.float(), v, p, s2, x_hat))
        latents, velocity, momentum, speed2, path_head = (torch.stack(t, 1) for t in zip(*nodes))
        speed = speed2.sqrt()
        done = torch.arange(steps, device=dev)[None, :] < taken[:, None]        # the steps a trajectory has taken
        length = h * torch.where(done, 0.5 * (speed[:, :-1] + speed[:, 1:]), torch.zeros_like(speed[:, 1:])).sum(1)
        x_data = to_data_space(self.chain, path_head.flatten(0, 1))
        return {"latents": latents, "velocity": velocity, "momentum": momentum, "speed2": speed2, "length": length,
                "path_head": path_head, "path": x_data.view(B, steps + 1, *x_data.shape[1:]), "steps_taken": taken, "info": info}

    # -- parallel transport --------------------------------------------------------------------
    @torch.no_grad()
    def transport_latents(self, latents, w):
        """Carry the latent tangent vectors ``w`` ((B, d) or (B, d, m), any m >= 1, floating point: components at point 0) along
        the curves ``latents`` (B, P, d) float32 of the head's latents, P >= 2 -- any curves, they need not be geodesics -- by
        parallel transport in the pull-back metric G = J^T J.  Per segment, with C_i = J_i^T J_{i+1}, in float64:
        forward = G_{i+1}^-1 C_i^T w_i (the projection onto the next tangent plane), backward = C_i^-1 G_i w_i (the inverse of the
        projection back), w_{i+1} = (forward + backward) / 2: the rotation between the two planes up to the fourth power of the
        angle between them.  Returns device tensors for the B curves of N = P - 1 segments:
          ``vectors`` (B, P, d, m) float64, the components at every point (``vectors[:, 0]`` = w); ``forward`` and ``backward``
          (B, N, d, m) float64 -- their gap shows how far the tangent plane turned in a segment; ``norm2`` (B, P, m) float64 =
          w_i^T G_i w_i, which parallel transport keeps; ``info`` (B,) int32: 0, 1 where a pivot of some G_{i+1} or C_i failed in
          segment i (``forward`` / ``backward`` from that segment on and ``vectors`` / ``norm2`` from point i + 1 on are NaN), 2
          where an input was not finite (everything NaN); the other curves are unaffected.  A (B, d) ``w`` gives m = 1.
        One decode sweep with tangents over every point -- in sub-batches of whole curves, each padded with a copy of its first and
        of its last point so that one ``engine.cross_gram`` call yields every in-curve block --, the Gram and cross-Gram launches
        and ``engine.transport_chain`` once per group of 16 vectors; enqueues kernels only -- no copy to the host, no
        synchronisation -- and leaves ``head.last_gram`` alone.  On ReLU couplers the manifold is piecewise linear: nothing
        converges with P there, the scheme just stays well behaved."""
        E.require_gpu(latents, "latents")
        prog = self.head.program
        d = prog.d
        if latents.dim() != 3 or latents.shape[2] != d or latents.shape[1] < 2:
            raise ValueError(f"latents {tuple(latents.shape)} must be (B, points >= 2, {d})")
        B, P = latents.shape[0], latents.shape[1]
        if not isinstance(w, torch.Tensor) or not w.is_floating_point() or w.device != latents.device or w.dim() not in (2, 3) or \
                w.shape[:2] != (B, d) or (w.dim() == 3 and w.shape[2] < 1):
            raise ValueError(f"w {tuple(getattr(w, 'shape', ()))} on {getattr(w, 'device', type(w).__name__)} must be ({B}, {d}) or "
                             f"({B}, {d}, m >= 1) floating point on {latents.device}")
        if B == 0:
            raise ValueError("transport needs at least one curve")
        w0 = (w[:, :, None] if w.dim() == 2 else w).double().transpose(1, 2).contiguous()       # (B, m, d)
        chunk = (prog.tangent_chunk(B * P + 2) - 2) // P
        if chunk <= 0:
            raise ValueError(f"points = {P}: one curve of {P} points and its two padding samples do not fit the sub-batch of "
                             f"{prog.tangent_chunk(B * P + 2)} samples a decode sweep may hold; use fewer points")
        with E.scope(self.head.kernels):
            parts = [self._transport(latents[i:i + chunk], w0[i:i + chunk]) for i in range(0, B, chunk)]
        return join_parts(parts)

    def _transport(self, latents, w0):
        prog = self.head.program
        B, P, d = latents.shape
        m = w0.shape[1]
        flat = latents.reshape(B * P, d)
        # one "curve" of B P + 2 points: its B P - 1 interior pairs are the pairs (s, s + 1) of the curve-major stack
        padded = torch.cat([flat[:1], flat, flat[-1:]])
        _, T = prog.decode(padded, tangents=True)
        jtj = E.gram_cholesky(T, d, 1).jtj[1:-1]
        cross = E.cross_gram(T, d, B * P + 2)[0]
        del T
        groups = [E.transport_chain(jtj, cross, w0[:, j:j + E.TRANSPORT_MAX_VECTORS].contiguous(), P)
                  for j in range(0, m, E.TRANSPORT_MAX_VECTORS)]
        join = lambda name: torch.cat([getattr(r, name) for r in groups], 2).transpose(2, 3).contiguous()
        out = {"vectors": join("out"), "forward": join("fwd"), "backward": join("bwd"),
               "norm2": torch.cat([r.norm2 for r in groups], 2), "info": groups[0].info}
        if len(groups) > 1:
            # the groups share the matrices, so they agree on code 1; a non-finite vector in one group is code 2 for the whole curve
            for r in groups[1:]:
                out["info"] = torch.maximum(out["info"], r.info)
            bad = out["info"] == 2
            for key in ("vectors", "forward", "backward", "norm2"):
                t = out[key]
                out[key] = torch.where(bad.view(-1, *([1] * (t.dim() - 1))), torch.full_like(t, float("nan")), t)
        return out

    @torch.no_grad()
    def transport(self, x0, x1, w, steps=None):
        """``connect(x0, x1, steps)`` and ``transport_latents`` of ``w`` ((B, d) or (B, d, m): latent components at ``x0``) along
        its relaxed ``latents``: the values of ``connect``, unchanged, beside ``vectors``, ``forward``, ``backward``, ``norm2``,
        ``transport_info`` (the ``info`` of ``transport_latents``; ``info`` stays ``connect``'s) and ``transported`` (B, d, m)
        float64 = ``vectors[:, -1]``, the components at ``x1``."""
        out = dict(self.connect(x0, x1, steps))
        tr = self.transport_latents(out["latents"], w)
        tr["transport_info"] = tr.pop("info")
        out.update(tr)
        out["transported"] = tr["vectors"][:, -1]
        return out

    @torch.no_grad()
    def analogy(self, xa, xb, xc, steps=None, shoot_steps=None, time=1.0):
        """"``xa`` is to ``xb`` as ``xc`` is to ?": the velocity v = ``log(xa, xb)["velocity"]`` that walks from ``xa`` to ``xb``
        is carried along the geodesic from ``xa`` to ``xc`` by ``transport`` and ``shoot``s from ``xc`` for ``time``.  Returns the
        values of ``shoot`` (``path[:, -1]`` is the answer in data space) beside ``velocity`` (B, d) float64, ``transported``
        (B, d) float64 -- that velocity at ``xc`` -- and ``transport_info`` (B,) int32."""
        v = self.log(xa, xb, steps)["velocity"]
        tr = self.transport(xa, xc, v, steps)
        moved = tr["transported"][:, :, 0].contiguous()
        out = dict(self.shoot(xc, moved, shoot_steps, time))
        out.update(velocity=v, transported=moved, transport_info=tr["transport_info"])
        return out
