"""Curvature of the learned manifold: the second fundamental form of the decoder's image in a frame of latent directions,
and from it -- by the Gauss equation, with no third derivative -- the Riemann tensor of the pull-back metric, sectional curvatures, the
frame's scalar curvature and the extrinsic curvature of straight latent lines.

The decoder g embeds the manifold in the flat input space of the head.  With J = dg, G = J^T J and the second derivative d2g,
    II(u, v) = (I - J G^-1 J^T) d2g[u, v]                                  the normal component of the second derivative
    R(u_a, u_b, u_c, u_d) = <II_ac, II_bd> - <II_ad, II_bc>                Gauss
and d2g[u_a, u_b] is a central difference of the direction sweep J(z +- h u_a) u_b.  Per sub-batch: one decode sweep with all d columns
at z (J, G), one 16-column sweep over the 2 m shifted latents and one float64 kernel per sample (csrc/second_form.hip), which forms the
symmetrised differences H_ab, their Gram matrix, its Schur complement N = H^T H - H^T J G^-1 J^T H -- the Gram matrix of the normal
components II_ab -- and the Christoffel contractions G^-1 J^T H_ab; nothing leaves the device.

    curv = cmf_amd.ManifoldCurvature(density)
    out = curv.at(x.cuda())                              # the first min(d, 4) latent axes as frame
    out["sectional"], out["scalar"]                      # (B, m, m) K_ab; (B,)
    out["normal_curvature"]                              # (B, m): how sharply the latent line along u_a bends in the head's space
    out["asymmetry"]                                     # (B,): ~1e-4 .. 1e-3 on smooth couplers; order 1 means "not a curvature"

On ReLU couplers the manifold is piecewise linear: the two estimates D_ab and D_ba of one mixed derivative disagree at every step, the
numbers returned are a finite-difference artefact at scale h, and ``asymmetry`` says so (order 1 instead of 1e-4 .. 1e-3).
"""
import math

import torch

from . import engine as E
from .metric_stats import metric_head
from .projection import ManifoldProjector, join_parts

__all__ = ["ManifoldCurvature"]


def pair_index(m):
    """(m, m) int64: the position of the pair (min(a, b), max(a, b)) among the q = m (m + 1) / 2 pairs a <= b in a-major order."""
    idx = torch.zeros(m, m, dtype=torch.int64)
    p = 0
    for a in range(m):
        for b in range(a, m):
            idx[a, b] = idx[b, a] = p
            p += 1
    return idx


def riemann_of(second_gram, m):
    """R_abcd = N[(a, c), (b, d)] - N[(a, d), (b, c)] (..., m, m, m, m) of the Gram matrix N (..., q, q) of the normal components."""
    P = pair_index(m).to(second_gram.device)
    ac, bd = P[:, None, :, None].expand(m, m, m, m), P[None, :, None, :].expand(m, m, m, m)
    ad, bc = P[:, None, None, :].expand(m, m, m, m), P[None, :, :, None].expand(m, m, m, m)
    return second_gram[..., ac, bd] - second_gram[..., ad, bc]


def spd_inverse(g):
    """The inverse of the small symmetric positive definite matrices ``g`` (..., m, m) by Gauss-Jordan elimination without pivoting, in
    elementwise torch operations (m <= 4: no solver library, no synchronisation).  A pivot that is not positive gives inf / NaN."""
    m = g.shape[-1]
    aug = torch.cat([g, torch.eye(m, dtype=g.dtype, device=g.device).expand_as(g)], -1).clone()
    for k in range(m):
        row = aug[..., k:k + 1, :] / aug[..., k:k + 1, k:k + 1]
        aug = aug - aug[..., :, k:k + 1] * row
        aug[..., k:k + 1, :] = row
    return aug[..., m:]


def curvatures(second_gram, frame_metric, stats, m):
    """The tensors the product derives from the kernel's outputs, in float64 torch operations: a dict of ``riemann``, ``sectional``,
    ``scalar``, ``normal_curvature``, ``asymmetry``, ``cancellation`` (see ``ManifoldCurvature.at_latents``)."""
    g, N = frame_metric, second_gram
    R = riemann_of(N, m)
    ar = torch.arange(m, device=N.device)
    diag = g[..., ar, ar]                                                    # (..., m)
    gg = diag[..., :, None] * diag[..., None, :]
    den = gg - g * g
    num = R[..., ar[:, None], ar[None, :], ar[:, None], ar[None, :]]        # R_abab
    K = torch.where(den > m * 2.0 ** -24 * gg, num / den, torch.full_like(den, float("nan")))
    K[..., ar, ar] = 0.0 * num[..., ar, ar]                                  # R_aaaa = x - x: 0, or NaN on a failed sample
    ginv = spd_inverse(g)
    scalar = torch.einsum("...ac,...bd,...abcd->...", ginv, ginv, R)
    P = pair_index(m).to(N.device)
    naa = N[..., P[ar, ar], P[ar, ar]]                                       # |II_aa|^2, clamped: rounding may leave it below zero
    normal = naa.clamp_min(0.0).sqrt() / diag
    # 0 only where the denominator IS zero (m = 1 included: both sums are then zero); the NaN sums of a failed sample stay NaN
    asym = torch.where(stats[..., 1] == 0, torch.zeros_like(stats[..., 0]), (stats[..., 0] / stats[..., 1]).sqrt())
    return {"riemann": R, "sectional": K, "scalar": scalar, "normal_curvature": normal, "asymmetry": asym,
            "cancellation": stats[..., 3] / stats[..., 2]}


class ManifoldCurvature:
    """Curvature of the manifold of a non-square density with latent dimension <= 128, in frames of up to 4 latent directions.

    ``step``: the finite-difference step h in latent units along a unit direction; None: ``DEFAULT_STEP``, the power of two at which
    the rounding error of a float32 decoder and the truncation error cross on the tanh-MLP fixtures."""

    #: chosen by the sweep of DESIGN 4.3m: the h in 2^-3 .. 2^-10 that minimises the worst relative error of N over the three MLP fixtures
    DEFAULT_STEP = 2.0 ** -7

    def __init__(self, density, step=None):
        self.density, self.head = density, metric_head(density, "latent", "manifold curvature")
        d = self.head.program.d
        if d > E.CURVATURE_MAX_WIDTH:
            raise ValueError(f"latent_dimension = {d}: manifold curvature supports 1 <= latent_dimension <= "
                             f"{E.CURVATURE_MAX_WIDTH} (DESIGN 9)")
        self.step = self._step(self.DEFAULT_STEP if step is None else step)
        # the encoder's latent under the head's one-shot pre-hook and the bijections in front of the head: the projector's
        self.projector = ManifoldProjector(density, steps=0)

    @staticmethod
    def _step(step):
        h = float(step)
        if not (h > 0 and math.isfinite(h)):
            raise ValueError(f"step must be finite and > 0, got {step}")
        return h

    @torch.no_grad()
    def at(self, x, directions=None, step=None):
        """``at_latents`` at the encoder's latents of ``x`` (the density's inputs, (B, *x_shape), as for ``elbo`` / ``ood``; never
        modified, no dequantisation noise is drawn)."""
        E._check_on_gpu("x", x)
        with E.scope(self.head.kernels):
            z = self.projector.head_input_and_latent(x)[1]
        return self.at_latents(z, directions, step)

    @torch.no_grad()
    def at_latents(self, z, directions=None, step=None):
        """The curvature of the manifold at the head's latents ``z`` (B, d) float32 in the frame ``directions``: (B, d, m), or (d, m)
        shared by the batch, floating point, 1 <= m <= min(d, 4) columns; None: the first min(d, 4) latent axes.  Every column is
        normalised to unit Euclidean latent length in float64 (a zero or non-finite column is a ValueError: the values are looked at
        where they are, which makes the call wait for them once); everything below refers to that ``frame`` u_0 .. u_{m-1}.  ``step``
        = h: the shifted latents are (z.double() +- h u_a).float(); None: the object's.  With q = m (m + 1) / 2 pairs (a, b), a <= b,
        a-major, H_ab the symmetrised central difference of J(z +- h u_a) u_b and G = J^T J, returns device tensors, float64 unless
        noted:
          ``frame`` (B, d, m); ``step`` (B,); ``frame_metric`` (B, m, m) = u_a^T G u_b;
          ``second_gram`` (B, q, q) = N, the Gram matrix <II_p, II_p'> of the normal components of the H_p;
          ``christoffel`` (B, q, d) = G^-1 J^T H_ab: the Christoffel symbols of the pull-back metric contracted with the frame -- the
            latent acceleration a geodesic along u_a must cancel;
          ``riemann`` (B, m, m, m, m): R_abcd = N[(a,c),(b,d)] - N[(a,d),(b,c)];
          ``sectional`` (B, m, m): K_ab = R_abab / (g_aa g_bb - g_ab^2) for a != b (in this sign convention R_abba = -R_abab), 0 on
            the diagonal, NaN where the denominator is <= m 2^-24 g_aa g_bb: the frame is then degenerate as far as a float32 G can tell;
          ``scalar`` (B,) = sum g^ac g^bd R_abcd with g^-1 the inverse of ``frame_metric``: the scalar curvature of the manifold when
            m = d, otherwise only the frame's partial contraction -- the scalar curvature of the m-dimensional slice spanned by the
            frame, as the Gauss equation sees it with the full normal space;
          ``normal_curvature`` (B, m) = sqrt(N[(a,a),(a,a)]) / g_aa: the extrinsic curvature, in the head's input space, of the
            straight latent line through z along u_a, its tangential acceleration excluded;
          ``asymmetry`` (B,) = sqrt(sum_{a<b} ||D_ab - D_ba||^2 / sum_{a<b} ||H_ab||^2), 0 for m = 1 or a zero denominator: the two
            one-sided estimates of every mixed derivative against their mean.  About 1e-4 .. 1e-3 on smooth (tanh) couplers at the
            default step; of order 1 on ReLU couplers, whose manifold is piecewise linear -- every number returned is then a
            finite-difference artefact at scale h and not a curvature;
          ``cancellation`` (B,) = trace N / trace H^T H: how much of the second derivative is normal (small values mean the Schur
            complement cancelled most of its digits);
          ``info`` (B,) int32, the code of ``engine.second_form``: 0 ok; 1 a pivot of G failed: ``second_gram``, ``christoffel`` and
            what derives from N -- ``riemann``, ``sectional`` (its diagonal too), ``scalar``, ``normal_curvature``, ``cancellation`` --
            are NaN, ``frame_metric`` and ``asymmetry`` are kept; 2 a non-finite value reached the kernel (a NaN latent, say): every
            result of the sample is NaN, ``asymmetry`` included, and only the inputs ``frame`` and ``step`` are returned as given.
            The other samples of the batch are not affected.
        Sub-batches of whole samples like the log-density path (a sample costs 2 m + 1 decodes); enqueues kernels only -- beyond the
        look at ``directions`` no copy to the host, no synchronisation -- and leaves ``head.last_gram`` alone."""
        prog = self.head.program
        d = prog.d
        E._check_on_gpu("z", z)
        if z.dim() != 2 or z.shape[1] != d or z.dtype != torch.float32:
            raise ValueError(f"z must be (B, {d}) float32, got {tuple(z.shape)} {z.dtype}")
        B, dev = z.shape[0], z.device
        if B == 0:
            raise ValueError("curvature needs at least one latent")
        h = self.step if step is None else self._step(step)
        if directions is None:
            directions = torch.eye(d, min(d, E.CURVATURE_MAX_FRAME), dtype=torch.float64, device=dev)
        E._check_on_gpu("directions", directions)
        if not directions.is_floating_point() or directions.device != dev or directions.dim() not in (2, 3) or \
                tuple(directions.shape[:-1]) not in ((B, d), (d,)):
            raise ValueError(f"directions must be a floating point tensor of shape ({B}, {d}, m) or ({d}, m) on {dev}, got "
                             f"{tuple(directions.shape)} {directions.dtype} on {directions.device}")
        m = directions.shape[-1]
        if not 1 <= m <= min(d, E.CURVATURE_MAX_FRAME):
            raise ValueError(f"m = {m}: a frame has 1 <= m <= min(d, {E.CURVATURE_MAX_FRAME}) = {min(d, E.CURVATURE_MAX_FRAME)} "
                             f"directions (DESIGN 9)")
        frame = directions.double()
        norm = (frame * frame).sum(-2, keepdim=True).sqrt()
        if not bool((torch.isfinite(norm) & (norm > 0)).all()):
            raise ValueError("every column of directions must be finite and not zero")
        frame = (frame / norm).expand(B, d, m).contiguous()
        chunk = prog.tangent_chunk(B * (2 * m + 1)) // (2 * m + 1)
        if chunk == 0:
            raise ValueError(f"m = {m}: one latent and its {2 * m} shifted copies do not fit the sub-batch of "
                             f"{prog.tangent_chunk(B * (2 * m + 1))} samples a decode sweep may hold; use fewer directions")
        with E.scope(self.head.kernels):
            parts = [self._at(z[i:i + chunk], frame[i:i + chunk], h) for i in range(0, B, chunk)]
        return join_parts(parts)

    def _at(self, z, frame, h):
        prog = self.head.program
        (B, d), m, dev = z.shape, frame.shape[2], z.device
        _, T = prog.decode(z.contiguous(), tangents=True)
        jtj = E.gram_cholesky(T, d, 1).jtj
        rows = frame.transpose(1, 2).contiguous()                                # (B, m, d)
        sign = torch.tensor([h, -h], dtype=torch.float64, device=dev)
        shifted = (z.double()[:, None, None, :] + sign[None, None, :, None] * rows[:, :, None, :]).float()      # (B, m, 2, d)
        eps = frame.float()[:, None, None].expand(B, m, 2, d, m).reshape(B * m * 2, d, m).contiguous()
        _, S = prog.decode(shifted.reshape(B * m * 2, d), tangents=True, eps=eps)
        step = torch.full((B,), h, dtype=torch.float64, device=dev)
        r = E.second_form(T, jtj, S, rows, step)
        out = {"frame": frame, "step": step, "frame_metric": r.frame_metric, "second_gram": r.second_gram,
               "christoffel": r.christoffel, "info": r.info}
        out.update(curvatures(r.second_gram, r.frame_metric, r.stats, m))
        return out
