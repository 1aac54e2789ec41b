"""Projection onto the learned manifold: how far an input is from the image of the decoder g, and the nearest point
on it.  ``ood()`` answers with the encoder's latent, ||y - g(e(y))||^2 -- an upper bound, because the encoder is a left inverse of
g, not the orthogonal projection, and the residual it leaves has a component inside the tangent space range(J).
``ManifoldProjector`` removes that component with a few damped Gauss-Newton (Levenberg-Marquardt) steps on z -> ||y - g(z)||^2,
started at the encoder's latent.  A step is one decode sweep (x_hat, J), the Gram kernel (J^T J) and one per-sample kernel
(csrc/gn_step.hip: J^T r and the float64 normal-equation solve); nothing leaves the device.

    proj = cmf_amd.ManifoldProjector(density, steps=10)
    out = proj.project(x.cuda())
    out["distance2"], out["initial_distance2"]          # squared distances in the head's input space, after and before
    out["tangential2"] / out["distance2"]               # share of the remaining residual that is still tangential
    proj.complete(x.cuda(), weights)                    # the same with missing or unevenly trusted elements
    proj.robust(x.cuda())["weights"]                    # the same with corrupt elements nobody marked: IRLS
    proj.recover(y, A, x_init=x0.cuda())                # the same seen through a linear measurement y = A x
    proj.recover(y, A, x_init=x0.cuda(), space="data")  # A acts on the density's input, e.g. pixel values
    proj.uncertainty(out, operator=A, space="data")     # error bars on any of these answers
"""
import torch

from . import engine as E
from .bijections import AffineBijection, Squeeze2dBijection, ViewBijection, _Elementwise
from .densities import BijectionDensity, DataParallelDensity, WrapperDensity
from .metric_stats import metric_head

__all__ = ["ManifoldProjector", "data_space_wrapper", "to_data_space_weights"]

#: ``robust``'s default tuning constants: 95 % efficiency at the normal distribution (Huber 1964; Beaton and Tukey 1974)
ROBUST_TUNING = {"huber": 1.345, "tukey": 4.685}

#: the clamps of the per-sample damping
DAMPING_MIN, DAMPING_MAX = 1e-12, 1e8


def wrapper_bijections(density, head):
    """The bijections between ``density`` and its ``head``, outermost first: what ``fixed_sample`` inverts on the way out."""
    chain, node = [], density
    while node is not head:
        if isinstance(node, BijectionDensity):
            chain.append(node.bijection)
            node = node.prior
        elif isinstance(node, WrapperDensity):
            node = node.density
        elif isinstance(node, DataParallelDensity):
            node = node.module
        else:
            raise NotImplementedError(f"manifold projection through a {type(node).__name__} in front of the head is not built")
    return chain


def to_data_space(chain, x):
    """The head-space tensor ``x`` mapped back to data space through the bijections ``chain`` (``wrapper_bijections``)."""
    for bijection in reversed(chain):
        x = bijection.z_to_x(x)["x"]
    return x


def to_head_space_weights(chain, w):
    """The per-element weights ``w`` (B, *data shape) mapped to the head's input space through the bijections ``chain``
    (``wrapper_bijections``): an elementwise bijection (logit, scalar multiplication / addition, affine) moves every element on its
    own and leaves the weights as they are -- the same tensor --, a reshaping one (``ViewBijection``, ``Squeeze2dBijection``)
    permutes them with the index map its own ``x_to_z`` applies to data.  Anything else: NotImplementedError."""
    for bijection in chain:
        if isinstance(bijection, (_Elementwise, AffineBijection)):
            continue
        if isinstance(bijection, ViewBijection):
            w = w.reshape(w.shape[0], *bijection.z_shape)
        elif isinstance(bijection, Squeeze2dBijection):
            x2z = bijection._maps.get("x2z", w.device).long()        # z[r] = x[x2z[r]]
            w = w.reshape(w.shape[0], -1).index_select(1, x2z).view(w.shape[0], *bijection.z_shape)
        else:
            raise NotImplementedError(f"weights cannot be carried through a {type(bijection).__name__} in front of the head: it "
                                      "mixes elements (only elementwise and reshaping bijections are built)")
    return w


def to_data_space_weights(chain, w):
    """The inverse index map of ``to_head_space_weights``: head-space per-element weights ``w`` (B, *head shape) taken back to the
    data layout through the bijections ``chain`` -- elementwise ones leave them as they are, a reshaping one undoes its
    permutation with the index map its own ``z_to_x`` applies.  Anything else: NotImplementedError."""
    for bijection in reversed(chain):
        if isinstance(bijection, (_Elementwise, AffineBijection)):
            continue
        if isinstance(bijection, ViewBijection):
            w = w.reshape(w.shape[0], *bijection.x_shape)
        elif isinstance(bijection, Squeeze2dBijection):
            z2x = bijection._maps.get("z2x", w.device).long()        # x[r] = z[z2x[r]]
            w = w.reshape(w.shape[0], -1).index_select(1, z2x).view(w.shape[0], *bijection.x_shape)
        else:
            raise NotImplementedError(f"weights cannot be carried through a {type(bijection).__name__} in front of the head: it "
                                      "mixes elements (only elementwise and reshaping bijections are built)")
    return w


def data_space_wrapper(chain):
    """The bijections ``chain`` (``wrapper_bijections``) as (wa, wc, logit, perm): the head's input is [logit](wa x + wc) of the
    data elements x, taken in the order ``perm`` -- head element r is data element perm[r]; ``perm`` is an int64 tensor on the
    host, or None for the flat order as it is.  Elementwise bijections fuse as the density's own fused pre-head fuses them
    (``BijectionDensity._fused_prehead``); a ``ViewBijection`` keeps the flat order and a ``Squeeze2dBijection`` contributes the
    index map its ``x_to_z`` applies to data (an index map commutes with what acts on every element alike, so it may stand
    anywhere in the chain).  An elementwise bijection after a logit, an ``AffineBijection`` (one scale per element: DESIGN 9) or
    any other type: NotImplementedError.  An empty chain gives (1.0, 0.0, False, None)."""
    wa, wc, logit, perm = 1.0, 0.0, False, None
    for bijection in chain:
        if isinstance(bijection, _Elementwise):
            if logit:
                raise NotImplementedError(f"a {type(bijection).__name__} after a logit in front of the head is not one fused "
                                          "pre-head wrapper: recover(space='data') is not built for it")
            wa, wc, logit = wa * bijection.a, wc * bijection.a + bijection.c, bool(bijection.logit)
        elif isinstance(bijection, ViewBijection):
            continue
        elif isinstance(bijection, Squeeze2dBijection):
            x2z = torch.from_numpy(bijection._maps._host["x2z"]).long()    # z[r] = x[x2z[r]]
            perm = x2z if perm is None else perm[x2z]
        else:
            raise NotImplementedError(f"recover(space='data') is not built for a {type(bijection).__name__} in front of the head "
                                      "(only scalar elementwise and reshaping bijections are)")
    if perm is not None and torch.equal(perm, torch.arange(perm.numel())):
        perm = None
    return wa, wc, logit, perm


def join_parts(parts):
    """The result dicts of a call's sub-batches as one dict, concatenated along the leading dimension."""
    return parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def refuse(name, t, want, fits):
    """``recover``'s and ``uncertainty``'s rule for a float32 argument -- dtype, shape, contiguity: said before the device is looked at."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not fits(t) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 {want} tensor, got {getattr(t, 'dtype', type(t).__name__)} "
                         f"{tuple(getattr(t, 'shape', ()))}"
                         f"{' (not contiguous)' if isinstance(t, torch.Tensor) and not t.is_contiguous() else ''}")


def noise_level(n_obs, d, cost=None, variance=None):
    """(sigma^2 (B,) float64, dof (B,) int32) of a least-squares fit of ``d`` parameters to ``n_obs`` (B,) observations: dof =
    n_obs - d and sigma^2 = ``variance`` where the caller knows it, else the residual estimate ``cost`` / dof -- NaN where dof <=
    0, set by ``torch.where`` on the tensors' own device (no look at the values)."""
    dof = (n_obs - d).to(torch.int32)
    if variance is not None:
        return variance, dof
    nan = torch.full_like(cost, float("nan"))
    return torch.where(dof > 0, cost / dof.clamp_min(1).to(cost.dtype), nan), dof


def wrapper_derivative(triple, x_hat):
    """|du/dv| (B, D) float32 at the head-space values ``x_hat`` of the fused pre-head v = [logit](wa x + wc) of ``triple`` (wa, wc,
    logit): (p (1 - p) if logit else 1) / |wa| with p the sigmoid of v, elementwise in float64 and through e = exp(-|v|) as the
    operator kernel forms it, p (1 - p) = e / (1 + e)^2 -- what ``engine.operator_apply_wrapped`` leaves in ``scale``,
    for the calls that run no operator kernel."""
    wa, _, logit = triple
    v = x_hat.flatten(1).double()
    if logit:
        e = torch.exp(-v.abs())
        return (e / (1.0 + e) ** 2 / abs(wa)).float()
    return torch.full_like(v, 1.0 / abs(wa)).float()


def lm_loop(state, cost, lam, steps, up, down, trial):
    """The accept/reject loop of the damped Gauss-Newton tools (the projector's samples, the geodesic's curves).  ``state``: a
    tuple of tensors with the unit -- sample or curve -- as leading dimension, of which ``state[cost]`` (units,) float64 is what the
    steps lower; ``lam`` (units,) float64, the dampings.  ``trial(state, lam)`` proposes: (solved (units,) bool, new state).  A
    unit accepts iff its solve succeeded and its cost strictly fell -- then it takes the new state, entry by entry, and lambda <-
    max(lambda ``down``, DAMPING_MIN) --, else it stays and lambda <- min(lambda ``up``, DAMPING_MAX).  Returns (state, lam,
    accepted (units,) int32, the steps each unit took)."""
    accepted = torch.zeros(lam.shape[0], dtype=torch.int32, device=lam.device)
    for _ in range(steps):
        solved, new = trial(state, lam)
        ok = solved & (new[cost] < state[cost])                       # a NaN cost compares false: rejected
        state = tuple(torch.where(ok.view(-1, *[1] * (s.dim() - 1)), n, s) for n, s in zip(new, state))
        lam = torch.where(ok, (lam * down).clamp_min(DAMPING_MIN), (lam * up).clamp_max(DAMPING_MAX))
        accepted += ok
    return state, lam, accepted


class ManifoldProjector:
    """Damped Gauss-Newton projection onto the manifold of a non-square density with latent dimension <= 128.

    ``steps`` iterations per call; every sample carries its own damping lambda, started at ``damping``: a step is accepted iff
    its solve succeeded and it strictly lowers the distance, then lambda <- max(lambda ``down``, 1e-12); otherwise the sample stays
    where it is and lambda <- min(lambda ``up``, 1e8).  The distance is therefore monotone non-increasing, and ``steps=0`` gives
    the diagnostics of the encoder's own latent."""

    def __init__(self, density, steps=10, damping=1e-3, up=10.0, down=0.1):
        self.density, self.head = density, metric_head(density, "latent", "manifold projection")
        d = self.head.program.d
        if d > E.PROJECT_MAX_WIDTH:
            raise ValueError(f"latent_dimension = {d}: the manifold projection supports 1 <= latent_dimension <= "
                             f"{E.PROJECT_MAX_WIDTH} (DESIGN 9)")
        if int(steps) < 0 or not damping >= 0 or not up >= 1 or not 0 < down <= 1:
            raise ValueError(f"need steps >= 0, damping >= 0, up >= 1 and 0 < down <= 1, got {steps}, {damping}, {up}, {down}")
        self.steps, self.damping, self.up, self.down = int(steps), float(damping), float(up), float(down)
        self.chain = wrapper_bijections(density, self.head)

    def head_input_and_latent(self, x):
        """(y, z): the head's input for ``x`` -- the space in which ``elbo`` / ``ood`` measure the reconstruction term -- and the
        encoder's latent, from ONE ``extract_latent`` call under a one-shot forward pre-hook on the head."""
        seen = []
        handle = self.head.register_forward_pre_hook(lambda module, args: seen.append(args))
        try:
            z = self.density.extract_latent(x, earliest_latent=False)
        finally:
            handle.remove()
        mode, y = seen[0][0], seen[0][1]
        assert len(seen) == 1 and mode == "extract-latent"
        return y.contiguous(), z.contiguous()

    def head_input(self, x):
        """The head's input for ``x``: the ``y`` of ``head_input_and_latent``, the space ``recover``'s operator acts on."""
        return self.head_input_and_latent(x)[0]

    def evaluate(self, y, z, lam):
        """Decode with tangents at ``z``, Gram, step kernel: the ``engine.GaussNewtonResult``."""
        prog = self.head.program
        x_hat, T = prog.decode(z, tangents=True)
        jtj = E.gram_cholesky(T, prog.d, 1).jtj
        return E.gauss_newton_step(T, jtj, y, x_hat.contiguous(), lam)

    @torch.no_grad()
    def project(self, x, steps=None):
        """Project every sample of ``x`` (the density's input, as for ``elbo`` / ``ood``; never modified, no dequantisation noise is
        drawn).  Returns device tensors for the B samples:
          ``latent`` (B, d) float32; ``reconstruction_head`` (B, *x_shape) = g(latent) in the head's input space and
          ``reconstruction``, the same mapped back to data space; ``distance2`` and ``initial_distance2`` (B,) float64, the squared
          distances ||y - g(z)||^2 at the returned and at the encoder's latent; ``tangential2`` (B,) float64 = g^T G^-1 g with
          g = J^T r at the returned latent, the part of ``distance2`` a better latent could still remove to first order (NaN
          where the closing ``info`` != 0); ``gradient`` (B, d) float64 = g; ``accepted`` (B,) int32, the steps taken; ``damping``
          (B,) float64, the final lambda; ``info`` (B,) int32, the code of the closing evaluation (``engine.gauss_newton_step``).
        Sub-batches like the log-density path; enqueues kernels only -- no copy to the host, no synchronisation -- and leaves
        ``head.last_gram`` alone."""
        E.require_gpu(x)
        steps = self.steps if steps is None else int(steps)
        prog, B = self.head.program, x.shape[0]
        if B == 0 or steps < 0:
            raise ValueError(f"project needs at least one sample and steps >= 0, got {B} samples and steps = {steps}")
        chunk = prog.tangent_chunk(B)
        with E.scope(self.head.kernels):
            parts = [self._project(x[i:i + chunk], steps) for i in range(0, B, chunk)]
        return join_parts(parts)

    def _project(self, x, steps):
        prog = self.head.program
        y, z = self.head_input_and_latent(x)

        def at(z):                                                    # the state of ``lm_loop``: (z, g(z), ||y - g(z)||^2)
            x_hat = prog.decode(z, tangents=False)[0].contiguous()
            return z, x_hat, E.residual_sqnorm(y, x_hat)[0]

        def trial(state, lam):
            r = self.evaluate(y, state[0], lam)
            solved = r.info == 0
            return solved, at(state[0] + torch.where(solved[:, None], r.delta, torch.zeros_like(r.delta)).float())

        state = at(z)
        d2_0 = state[2].clone()
        lam = torch.full((x.shape[0],), self.damping, dtype=torch.float64, device=x.device)
        (z, x_hat, d2), lam, accepted = lm_loop(state, 2, lam, steps, self.up, self.down, trial)
        r = self.evaluate(y, z, torch.zeros_like(lam))
        return {"latent": z, "reconstruction_head": x_hat, "reconstruction": to_data_space(self.chain, x_hat), "distance2": d2,
                "initial_distance2": d2_0, "tangential2": r.stats[:, 1].contiguous(), "gradient": r.grad, "accepted": accepted,
                "damping": lam, "info": r.info}

    def evaluate_weighted(self, w, y, z, lam):
        """Decode with tangents at ``z`` and the weighted step kernel: the ``engine.WeightedGaussNewtonResult``."""
        prog = self.head.program
        x_hat, T = prog.decode(z, tangents=True)
        return E.weighted_gauss_newton_step(T, w, y, x_hat.contiguous(), lam, d=prog.d)

    @torch.no_grad()
    def complete(self, x, weights, steps=None, init=None):
        """Weighted projection: minimise sum_i w_i (y_i - g(z)_i)^2 over z for every sample -- the projection of an
        input with missing (w_i = 0) or unevenly trusted elements; g(z) at the elements with w_i = 0 is the imputation.
          ``x``: as for ``project``, finite everywhere; its values where the weight is zero only choose the starting latent (the
          encoder needs every element).  ``weights``: x's shape, or broadcastable over the batch ((*x.shape[1:]) or (1,
          *x.shape[1:])); floating point or bool, on x's device, >= 0.  They are carried to the head's input space through the
          wrapper chain (``to_head_space_weights``), where the cost is measured -- as ``distance2`` is.  ``init``: optional (B, d)
          float32 starting latent instead of the encoder's.
        The loop is ``project``'s -- the same dampings, clamps and strict ``<`` acceptance, on the weighted cost, with a closing
        evaluation at lambda = 0 -- and so are the returned keys, except: ``cost`` and ``initial_cost`` (B,) float64 in place of the
        distances; ``tangential2`` and ``gradient`` from the weighted system; ``distance2``, the unweighted ||y - g(z)||^2 over ALL
        elements, as a diagnostic; ``observed`` (B,) int32, the elements with w > 0.
        Whether a weight is negative or not finite is the kernel's finding, not a host look: such a sample never accepts a step
        and closes with ``info`` = 2 and NaN costs.  The iteration converges from the encoder's latent of a mildly wrong input with
        clearly more observed elements than 2 d; from a harsher start -- another sample's values in the hidden elements, or fewer
        observed elements than about 2 d -- samples can end in a local minimum or on a singular weighted Gram matrix (``info`` = 1).
        Sub-batches like ``project``; enqueues kernels only, and leaves ``head.last_gram`` alone."""
        steps = self.steps if steps is None else int(steps)
        prog, B = self.head.program, x.shape[0]
        if B == 0 or steps < 0:
            raise ValueError(f"complete needs at least one sample and steps >= 0, got {B} samples and steps = {steps}")
        if not isinstance(weights, torch.Tensor) or not (weights.is_floating_point() or weights.dtype == torch.bool):
            raise ValueError(f"weights must be a floating point or bool tensor, got {getattr(weights, 'dtype', type(weights).__name__)}")
        if tuple(weights.shape) not in (tuple(x.shape), tuple(x.shape[1:]), (1, *x.shape[1:])):
            raise ValueError(f"weights must have x's shape {tuple(x.shape)} or broadcast over its batch, got {tuple(weights.shape)}")
        if init is not None and (not isinstance(init, torch.Tensor) or init.dtype != torch.float32 or tuple(init.shape) != (B, prog.d)):
            raise ValueError(f"init must be a float32 ({B}, {prog.d}) tensor, got {getattr(init, 'dtype', type(init).__name__)} "
                             f"{tuple(getattr(init, 'shape', ()))}")
        to_head_space_weights(self.chain, torch.empty(1, *x.shape[1:]))                # refuses what cannot be mapped, before any launch
        for name, v in (("weights", weights), ("init", init)):
            if v is not None and v.device != x.device:
                raise ValueError(f"{name} must be on x's device {x.device}, got {v.device} (there is no CPU fallback)")
        E.require_gpu(x)
        w = weights.to(torch.float32).expand(x.shape)
        chunk = prog.tangent_chunk(B)
        with E.scope(self.head.kernels):
            parts = [self._complete(x[i:i + chunk], w[i:i + chunk], steps, None if init is None else init[i:i + chunk])
                     for i in range(0, B, chunk)]
        return join_parts(parts)

    def _complete(self, x, w, steps, init):
        prog = self.head.program
        y, z = self.head_input_and_latent(x)
        if init is not None:
            z = init.contiguous().clone()
        w = to_head_space_weights(self.chain, w).reshape(y.shape).contiguous()

        def at(z):                                                    # the state of ``lm_loop``: (z, g(z), sum w (y - g(z))^2)
            x_hat = prog.decode(z, tangents=False)[0].contiguous()
            return z, x_hat, E.weighted_residual_sqnorm(w, y, x_hat)[0]

        def trial(state, lam):
            r = self.evaluate_weighted(w, y, state[0], lam)
            solved = r.info == 0
            return solved, at(state[0] + torch.where(solved[:, None], r.delta, torch.zeros_like(r.delta)).float())

        state = at(z)
        c_0 = state[2].clone()
        lam = torch.full((x.shape[0],), self.damping, dtype=torch.float64, device=x.device)
        (z, x_hat, c), lam, accepted = lm_loop(state, 2, lam, steps, self.up, self.down, trial)
        r = self.evaluate_weighted(w, y, z, torch.zeros_like(lam))
        return {"latent": z, "reconstruction_head": x_hat, "reconstruction": to_data_space(self.chain, x_hat), "cost": c,
                "initial_cost": c_0, "tangential2": r.stats[:, 1].contiguous(), "gradient": r.grad,
                "distance2": E.residual_sqnorm(y, x_hat)[0], "observed": (w > 0).flatten(1).sum(1).to(torch.int32),
                "accepted": accepted, "damping": lam, "info": r.info}

    @torch.no_grad()
    def robust(self, x, loss="huber", tuning=None, scale=None, weights=None, steps=None, rounds=1, init=None):
        """Robust projection: the projection of an input of which some elements are grossly wrong and nobody knows
        which -- salt-and-pepper pixels, an occluder nobody masked.  Minimises 2 s^2 sum_i p_i rho((y_i - g(z)_i) / s) over z by
        iteratively reweighted least squares: every iteration is ``complete``'s weighted step with the weights w_i = p_i omega(r_i
        / s) of the current residual, from one per-sample kernel (``engine.robust_weights``) that also gives the robust cost.
          ``loss``: "huber" (convex: omega = min(1, c / |u|)) or "tukey" (the redescending biweight: omega = max(0, 1 - (u / c)^2)^2,
          exactly zero beyond c).  ``tuning``: c > 0; None: 1.345 / 4.685, the textbook constants of 95 % efficiency at the normal
          distribution.  ``scale``: s, the noise standard deviation of the good elements in the head's input space -- a float > 0
          or a (B,) floating point tensor on x's device, held throughout (needs ``rounds`` == 1); None: estimated per sample as
          1.4826 x the exact lower median of |y - g(z)| over the used elements, at the latent a round starts from, and held for
          that round's ``steps`` iterations -- so the cost is monotone within a round.  ``rounds`` > 1 re-estimates s at the
          current latent and starts the damping anew.  ``weights``: optional known weights p, exactly as ``complete`` takes them
          (None: all one).  ``init``: optional (B, d) float32 starting latent instead of the encoder's.
        The loop is ``complete``'s -- the same dampings, clamps and strict ``<`` acceptance, a closing evaluation at lambda = 0 with
        the final weights, the same number of launches per iteration -- and so are the returned keys, plus: ``weights`` (B,
        *x.shape[1:]) float32, the final p omega in the data layout (``to_data_space_weights``): the outlier map; ``scale`` (B,)
        float64, s; ``effective`` (B,) float64 = sum_i omega_i.  ``cost`` and ``initial_cost`` are the robust cost at the end and
        at the start of the LAST round, under that round's scale: ``cost`` <= ``initial_cost`` always.  ``accepted`` sums over the
        rounds.  ``info``: the closing step's code, or the weights kernel's where that failed: 2 (a negative or non-finite weight
        or value), 3 (no scale: no used element, or more than half of the residuals exactly zero) -- such a sample never moves.
        A redescending loss has local minima and is best started from a convex one: ``robust(x, loss="tukey",
        init=robust(x)["latent"])``.  ``uncertainty(result, weights=result["weights"], noise_std=result["scale"])`` gives the usual
        IRLS approximation of the covariance (the weights taken as known), not the sandwich estimator.
        What to expect, measured on the float64 reference loop (tests/test_robust_host.py): the method needs
        redundancy, D >> d.  On the image fixtures (D = 784 with d = 5, D = 3072 with d = 6) at a 10 % share of outliers of 3 .. 6
        RMS it lands where ``complete`` with the true mask lands -- WHERE the start is fair: the encoder is not robust, and from
        its latent of the corrupted input the loop reaches the true point's basin on about half of the seeded problems; elsewhere
        it stalls where ``project`` stalls and finds no outlier (``rounds`` does not help, a better ``init`` does).  On the
        tabular configurations (D = 21, d = 10 and D = 6, d = 2) the reference loop cannot separate outliers from the manifold's
        own freedom even from the true latent, and at d = 4 on the 28 x 28 fixture it mostly fails at a 10 % share even from the
        true latent and succeeds at 3 %.
        Sub-batches like ``project``; enqueues kernels only -- no copy to the host, no synchronisation --, modifies no input and
        leaves ``head.last_gram`` alone."""
        steps = self.steps if steps is None else int(steps)
        prog, B = self.head.program, x.shape[0]
        if B == 0 or steps < 0:
            raise ValueError(f"robust needs at least one sample and steps >= 0, got {B} samples and steps = {steps}")
        if loss not in ROBUST_TUNING:
            raise ValueError(f"loss must be one of {sorted(ROBUST_TUNING)}, got {loss!r}")
        tuning = ROBUST_TUNING[loss] if tuning is None else float(tuning)
        if not tuning > 0:
            raise ValueError(f"tuning must be > 0, got {tuning}")
        if int(rounds) != rounds or rounds < 1:
            raise ValueError(f"rounds must be a whole number >= 1, got {rounds}")
        if scale is not None and rounds != 1:
            raise ValueError(f"a given scale is held throughout: it needs rounds == 1, got rounds = {rounds}")
        if isinstance(scale, torch.Tensor):
            if not scale.is_floating_point() or tuple(scale.shape) != (B,):
                raise ValueError(f"scale must be a float > 0 or a floating point ({B},) tensor, got {scale.dtype} {tuple(scale.shape)}")
        elif scale is not None and not float(scale) > 0:
            raise ValueError(f"scale must be > 0, got {scale}")
        if weights is not None:
            if not isinstance(weights, torch.Tensor) or not (weights.is_floating_point() or weights.dtype == torch.bool):
                raise ValueError(f"weights must be a floating point or bool tensor, got "
                                 f"{getattr(weights, 'dtype', type(weights).__name__)}")
            if tuple(weights.shape) not in (tuple(x.shape), tuple(x.shape[1:]), (1, *x.shape[1:])):
                raise ValueError(f"weights must have x's shape {tuple(x.shape)} or broadcast over its batch, got {tuple(weights.shape)}")
        if init is not None and (not isinstance(init, torch.Tensor) or init.dtype != torch.float32 or tuple(init.shape) != (B, prog.d)):
            raise ValueError(f"init must be a float32 ({B}, {prog.d}) tensor, got {getattr(init, 'dtype', type(init).__name__)} "
                             f"{tuple(getattr(init, 'shape', ()))}")
        to_head_space_weights(self.chain, torch.empty(1, *x.shape[1:]))                # refuses what cannot be mapped, before any launch
        for name, v in (("weights", weights), ("init", init), ("scale", scale)):
            if isinstance(v, torch.Tensor) and v.device != x.device:
                raise ValueError(f"{name} must be on x's device {x.device}, got {v.device} (there is no CPU fallback)")
        E.require_gpu(x)
        w = None if weights is None else weights.to(torch.float32).expand(x.shape)
        if scale is not None:
            scale = scale.double() if isinstance(scale, torch.Tensor) else torch.full((B,), float(scale), dtype=torch.float64,
                                                                                      device=x.device)
        chunk = prog.tangent_chunk(B)
        pick = lambda t, i: None if t is None else t[i:i + chunk]
        with E.scope(self.head.kernels):
            parts = [self._robust(x[i:i + chunk], pick(w, i), loss, tuning, pick(scale, i), steps, int(rounds), pick(init, i))
                     for i in range(0, B, chunk)]
        return join_parts(parts)

    def _robust(self, x, p, loss, tuning, scale, steps, rounds, init):
        prog = self.head.program
        y, z = self.head_input_and_latent(x)
        if init is not None:
            z = init.contiguous().clone()
        if p is not None:
            p = to_head_space_weights(self.chain, p).reshape(y.shape).contiguous()

        def weigh(z, x_hat, s):            # the state of ``lm_loop``: (z, g(z), robust cost, w, sum omega, the weights kernel's info)
            r = E.robust_weights(y, x_hat, loss, tuning, prior=p, scale=s)
            return (z, x_hat, r.cost, r.w, r.effective, r.info), r.scale

        def trial(state, lam):
            r = self.evaluate_weighted(state[3], y, state[0], lam)
            solved = r.info == 0
            z_new = state[0] + torch.where(solved[:, None], r.delta, torch.zeros_like(r.delta)).float()
            return solved, weigh(z_new, prog.decode(z_new, tangents=False)[0].contiguous(), s)[0]

        x_hat = prog.decode(z, tangents=False)[0].contiguous()
        accepted = torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)
        for _ in range(rounds):
            # a round's scale: the user's, or the estimate at the latent the round starts from -- then held (scale_in) by ``trial``
            state, s = weigh(z, x_hat, None if scale is None else scale.contiguous())
            s = s.contiguous()
            c_0 = state[2].clone()
            lam = torch.full((x.shape[0],), self.damping, dtype=torch.float64, device=x.device)
            state, lam, taken = lm_loop(state, 2, lam, steps, self.up, self.down, trial)
            z, x_hat = state[0], state[1]
            accepted += taken
        z, x_hat, c, w, effective, w_info = state
        r = self.evaluate_weighted(w, y, z, torch.zeros_like(lam))
        observed = torch.full_like(accepted, y[0].numel()) if p is None else (p > 0).flatten(1).sum(1).to(torch.int32)
        return {"latent": z, "reconstruction_head": x_hat, "reconstruction": to_data_space(self.chain, x_hat), "cost": c.contiguous(),
                "initial_cost": c_0, "tangential2": r.stats[:, 1].contiguous(), "gradient": r.grad,
                "distance2": E.residual_sqnorm(y, x_hat)[0], "observed": observed, "accepted": accepted, "damping": lam,
                "info": torch.where(w_info != 0, w_info, r.info), "weights": to_data_space_weights(self.chain, w).reshape(x.shape),
                "scale": s, "effective": effective.contiguous()}

    def evaluate_through(self, a, y, z, lam, apply=E.operator_apply):
        """Decode with tangents at ``z``, the operator kernel ``apply(T, a, x_hat)`` -> (K, yhat), Gram, step kernel on (K, yhat,
        y): the ``engine.GaussNewtonResult``."""
        prog = self.head.program
        x_hat, T = prog.decode(z, tangents=True)
        K, y_hat = apply(T, a, x_hat.contiguous())
        jtj = E.gram_cholesky(K, prog.d, 1).jtj
        return E.gauss_newton_step(K, jtj, y, y_hat, lam)

    @torch.no_grad()
    def recover(self, measurements, operator, init=None, x_init=None, steps=None, space="head"):
        """Linear inverse problem on the manifold: minimise ||y - A g(z)||^2 over z for every sample, where the
        input is seen only through the linear measurement y = A x.
          ``operator``: A, (M, D) float32, contiguous, on the GPU, shared by the batch; D is the number of elements of the head's
          input per sample, and A acts on the flattened HEAD-SPACE tensor in the element order of ``reconstruction_head.flatten(1)``
          -- the space in which ``distance2`` and ``complete``'s cost are measured (``head_input(x)`` maps an input there; an
          affine wrapper in front of the head can be folded into A and y by the caller).  ``measurements``: y, (B, M) float32 on
          the same device.  The starting latent is ``init`` (B, d) float32 as it is, else the encoder's latent of ``x_init`` (a
          tensor like the density's input: a crude back-projection of y), else zeros, the base density's mode; giving both is a
          ValueError.
        The loop is ``project``'s -- the same dampings, clamps and strict ``<`` acceptance, a closing evaluation at lambda = 0 --
        on the measured cost: a step is the decode sweep, the operator kernel (K = A J and yhat = A g(z), neither leaves the
        device), and the Gram and step kernels on (K, yhat, y) with M rows in place of D.  Returned keys as ``project``'s, except:
        ``measurement`` (B, M) float32 = A g(latent); ``cost`` and ``initial_cost`` (B,) float64 = ||y - A g(z)||^2 in place of
        the distances; ``tangential2`` and ``gradient`` from the measured system.
        With M < d the problem is underdetermined: the Marquardt term still makes every damped step solvable, so the cost falls,
        but K^T K is singular and the closing evaluation at lambda = 0 reports ``info`` = 1 with NaN ``tangential2`` -- a result,
        not an error; ``latent`` is one of the minimisers the damping picked.
          ``space`` = "data" (DESIGN 4.3p): A acts on the density's INPUT instead -- pixel values, flattened as ``x.flatten(1)``,
        ``measurements`` = A x --, which is what a blur or a down-sampling is linear in (``cmf_amd.operators`` builds both).
        The wrapper chain in front of the head must reduce to one fused pre-head v = [logit](wa x + wc) and an index map
        (``data_space_wrapper``; NotImplementedError otherwise).  The loop and the keys are the same; the operator kernel takes
        the wrapper along: yhat = A u(g(z)) with u the wrapper's inverse in float64, K = A diag(du/dv) J.  ``measurement`` = A
        u(g(latent)) with u in float64 (not A applied to the float32 ``reconstruction`` tensor), and ``cost`` and
        ``initial_cost`` are measured in data-space measurements.  Where the map reorders elements the columns of A are permuted
        once per call, on the device, into a copy.  With no wrapper (the tabular configurations) both spaces give the same bits.
        Sub-batches like ``project``; enqueues kernels only, modifies no input and leaves ``head.last_gram`` alone."""
        steps = self.steps if steps is None else int(steps)
        prog = self.head.program
        if space not in ("head", "data"):
            raise ValueError(f"space must be 'head' or 'data', got {space!r}")
        wrapper = data_space_wrapper(self.chain) if space == "data" else None
        D = 1
        for n in self.head.x_shape:
            D *= int(n)

        refuse("operator", operator, f"(M, {D})", lambda t: t.dim() == 2 and t.shape[0] >= 1 and t.shape[1] == D)
        M, dev = operator.shape[0], operator.device
        refuse("measurements", measurements, f"(B, {M})", lambda t: t.dim() == 2 and t.shape[1] == M)
        B = measurements.shape[0]
        if B == 0 or steps < 0:
            raise ValueError(f"recover needs at least one sample and steps >= 0, got {B} samples and steps = {steps}")
        if init is not None and x_init is not None:
            raise ValueError("give init (a starting latent) or x_init (an input to encode), not both")
        if init is not None:
            refuse("init", init, f"({B}, {prog.d})", lambda t: tuple(t.shape) == (B, prog.d))
        if x_init is not None and (not isinstance(x_init, torch.Tensor) or x_init.dim() < 2 or x_init.shape[0] != B):
            raise ValueError(f"x_init must hold the {B} samples of measurements, got {tuple(getattr(x_init, 'shape', ()))}")
        for name, v in (("measurements", measurements), ("init", init), ("x_init", x_init)):
            if v is not None and v.device != dev:
                raise ValueError(f"{name} must be on operator's device {dev}, got {v.device} (there is no CPU fallback)")
        E._check_on_gpu("operator", operator)
        if wrapper is not None and wrapper[3] is not None:
            operator = operator.index_select(1, wrapper[3].to(dev))       # acts on head-ordered elements; a copy
        chunk = prog.tangent_chunk(B)
        with E.scope(self.head.kernels):
            parts = [self._recover(measurements[i:i + chunk], operator, None if init is None else init[i:i + chunk],
                                   None if x_init is None else x_init[i:i + chunk], steps, *self._operator_calls(wrapper))
                     for i in range(0, B, chunk)]
        return join_parts(parts)

    @staticmethod
    def _operator_calls(wrapper):
        """(image(a, x_hat) -> yhat, apply(T, a, x_hat) -> (K, yhat)) of one sub-batch: the head-space operator kernel, or
        (``wrapper`` from ``data_space_wrapper``) the data-space one with one ``scale`` buffer that every step writes anew."""
        if wrapper is None:
            return E.operator_image, E.operator_apply
        triple, held = wrapper[:3], []

        def apply(T, a, x_hat):
            K, y_hat, scale = E.operator_apply_wrapped(T, a, x_hat, triple, held[0] if held else None)
            held[:] = [scale]
            return K, y_hat
        return (lambda a, x_hat: E.operator_image_wrapped(a, x_hat, triple)), apply

    def _recover(self, y, a, init, x_init, steps, image, apply):
        prog = self.head.program
        if init is not None:
            z = init.contiguous().clone()
        elif x_init is not None:
            z = self.head_input_and_latent(x_init)[1]
        else:
            z = torch.zeros(y.shape[0], prog.d, dtype=torch.float32, device=y.device)
        y = y.contiguous()

        def at(z):                                                    # the state of ``lm_loop``: (z, g(z), A g(z), ||y - A g(z)||^2)
            x_hat = prog.decode(z, tangents=False)[0].contiguous()
            y_hat = image(a, x_hat)
            return z, x_hat, y_hat, E.residual_sqnorm(y, y_hat)[0]

        def trial(state, lam):
            r = self.evaluate_through(a, y, state[0], lam, apply)
            solved = r.info == 0
            return solved, at(state[0] + torch.where(solved[:, None], r.delta, torch.zeros_like(r.delta)).float())

        state = at(z)
        c_0 = state[3].clone()
        lam = torch.full((y.shape[0],), self.damping, dtype=torch.float64, device=y.device)
        (z, x_hat, y_hat, c), lam, accepted = lm_loop(state, 3, lam, steps, self.up, self.down, trial)
        r = self.evaluate_through(a, y, z, torch.zeros_like(lam), apply)
        return {"latent": z, "reconstruction_head": x_hat, "reconstruction": to_data_space(self.chain, x_hat), "measurement": y_hat,
                "cost": c, "initial_cost": c_0, "tangential2": r.stats[:, 1].contiguous(), "gradient": r.grad,
                "accepted": accepted, "damping": lam, "info": r.info}

    @torch.no_grad()
    def uncertainty(self, result, weights=None, operator=None, space="head", noise_std=None):
        """Error bars of a fit: the classical first-order covariance of the nonlinear least-squares estimate that
        ``project``, ``complete`` or ``recover`` returned, under the model y = A u(g(z_0)) + eps with independent eps_i ~ N(0,
        sigma^2 / w_i) -- A the identity and w = 1 where the call had neither.  With J the decoder's Jacobian at the returned
        latent and N the call's normal matrix (J^T J, J^T diag(w) J, or K^T K with K = A diag(du/dv) J),
            cov(z) = sigma^2 N^-1,     var(g(z)_i) = sigma^2 j_i^T N^-1 j_i     (the delta method),
        computed per sample in float64 by one decode sweep, the call's own Gram kernel and ``engine.tangent_leverage``.
          ``result``: the dict of the call being qualified; ``latent`` is read, and -- with ``noise_std`` None -- ``cost``, or
          ``distance2`` where there is no ``cost``.  ``weights``: exactly as ``complete`` took them (shape, dtype, device, carried
          through ``to_head_space_weights``).  ``operator``, ``space``: exactly as ``recover`` took them (the same refusals; for
          "data" the same ``data_space_wrapper`` and column permutation).  Giving both ``weights`` and ``operator`` is a ValueError.
          ``noise_std``: sigma, the noise standard deviation per unit weight in the space the cost is measured in; a float >= 0
          or a (B,) floating point tensor on the device (a negative entry gives that sample NaN, on the device).  None: sigma^2 is
          estimated as cost / dof with dof = n_obs - d, n_obs = D for ``project``, the sample's count of w > 0 for ``complete``,
          M for ``recover``; NaN where dof <= 0.
        Returns device tensors: ``latent_covariance`` (B, d, d) float64 = sigma^2 N^-1; ``latent_std`` (B, d) float64, the root of
        its diagonal; ``leverage`` (B, *x_shape) float64 = j_i^T N^-1 j_i; ``reconstruction_std_head`` (B, *x_shape) float32 =
        sigma sqrt(leverage); with ``space`` = "data" also ``reconstruction_std`` (B, *data shape) float32 = |du/dv| times the
        head-space value, mapped back through the wrapper's index map (the delta method once more); ``noise_variance`` (B,)
        float64; ``dof`` (B,) int32; ``info`` (B,) int32, the kernel's: 0, 1 a singular normal matrix, 2 a non-finite input
        (covariance and leverage NaN in both cases).
        What the numbers are: the uncertainty of the MANIFOLD POINT, not a predictive interval for a new noisy observation
        (which would add sigma^2 / w_i).  An element the fit never saw (w_i = 0, or outside A's support) gets a finite value: how
        well the observed ones pin it down through the manifold.  With M < d, or fewer observed elements than d, the normal
        matrix is singular: ``info`` = 1 and NaN -- a result, as in ``recover``.  The covariance is first order: on ReLU
        couplers J is the Jacobian of the current linear piece and kinks are ignored (the caveat of DESIGN 4.3h), and no prior on
        z enters.
        Sub-batches like ``project``; enqueues kernels only -- no copy to the host --, modifies no input and leaves
        ``head.last_gram`` alone."""
        prog = self.head.program
        d = prog.d
        if space not in ("head", "data"):
            raise ValueError(f"space must be 'head' or 'data', got {space!r}")
        if weights is not None and operator is not None:
            raise ValueError("give weights (the problem of complete) or operator (the problem of recover), not both")
        wrapper = data_space_wrapper(self.chain) if space == "data" else None
        D = 1
        for n in self.head.x_shape:
            D *= int(n)
        latent = result.get("latent") if isinstance(result, dict) else None
        refuse("result['latent']", latent, f"(B, {d})", lambda t: t.dim() == 2 and t.shape[1] == d)
        B, dev = latent.shape[0], latent.device
        if B == 0:
            raise ValueError("uncertainty needs at least one sample, got 0")
        cost = variance = None
        if noise_std is None:
            cost = result.get("cost", result.get("distance2"))
            if not isinstance(cost, torch.Tensor) or cost.dtype != torch.float64 or tuple(cost.shape) != (B,):
                raise ValueError(f"result['cost'] (or 'distance2') must be a float64 ({B},) tensor when noise_std is None, got "
                                 f"{getattr(cost, 'dtype', type(cost).__name__)} {tuple(getattr(cost, 'shape', ()))}")
        elif isinstance(noise_std, torch.Tensor):
            if not noise_std.is_floating_point() or tuple(noise_std.shape) != (B,):
                raise ValueError(f"noise_std must be a float or a floating point ({B},) tensor, got {noise_std.dtype} "
                                 f"{tuple(noise_std.shape)}")
        elif not float(noise_std) >= 0:
            raise ValueError(f"noise_std must be >= 0, got {noise_std}")
        data_shape = None
        if weights is not None:
            if not isinstance(weights, torch.Tensor) or not (weights.is_floating_point() or weights.dtype == torch.bool):
                raise ValueError(f"weights must be a floating point or bool tensor, got "
                                 f"{getattr(weights, 'dtype', type(weights).__name__)}")
            data_shape = self.data_shape()
            if tuple(weights.shape) not in ((B, *data_shape), data_shape, (1, *data_shape)):
                raise ValueError(f"weights must have x's shape {(B, *data_shape)} or broadcast over its batch, got "
                                 f"{tuple(weights.shape)}")
            to_head_space_weights(self.chain, torch.empty(1, *data_shape))             # refuses what cannot be mapped
        if operator is not None:
            refuse("operator", operator, f"(M, {D})", lambda t: t.dim() == 2 and t.shape[0] >= 1 and t.shape[1] == D)
        for name, v in (("result['cost']", cost), ("noise_std", noise_std), ("weights", weights), ("operator", operator)):
            if isinstance(v, torch.Tensor) and v.device != dev:
                raise ValueError(f"{name} must be on result['latent']'s device {dev}, got {v.device} (there is no CPU fallback)")
        E._check_on_gpu("result['latent']", latent)
        if noise_std is not None:
            ns = noise_std.double() if isinstance(noise_std, torch.Tensor) else torch.full((B,), float(noise_std),
                                                                                         dtype=torch.float64, device=dev)
            variance = torch.where(ns >= 0, ns * ns, torch.full_like(ns, float("nan")))
        if wrapper is not None:
            data_shape = self.data_shape() if data_shape is None else data_shape
            if operator is not None and wrapper[3] is not None:
                operator = operator.index_select(1, wrapper[3].to(dev))   # acts on head-ordered elements; a copy
        w = None if weights is None else weights.to(torch.float32).expand(B, *data_shape)
        chunk = prog.tangent_chunk(B)
        pick = lambda t, i: None if t is None else t[i:i + chunk]
        with E.scope(self.head.kernels):
            parts = [self._uncertainty(latent[i:i + chunk], pick(w, i), operator, wrapper, data_shape, pick(cost, i),
                                       pick(variance, i)) for i in range(0, B, chunk)]
        return join_parts(parts)

    def data_shape(self):
        """The shape of one sample of the density's input: the head's ``x_shape`` taken back through the reshaping bijections of
        the wrapper chain (elementwise ones keep the shape)."""
        shape = tuple(int(n) for n in self.head.x_shape)
        for bijection in reversed(self.chain):
            if isinstance(bijection, (ViewBijection, Squeeze2dBijection)):
                shape = tuple(int(n) for n in bijection.x_shape)
        return shape

    def _uncertainty(self, z, w, a, wrapper, data_shape, cost, variance):
        prog = self.head.program
        d, Bc, dev = prog.d, z.shape[0], z.device
        x_hat, T = prog.decode(z.contiguous(), tangents=True)
        x_hat = x_hat.contiguous()
        scale = None
        if w is not None:
            w = to_head_space_weights(self.chain, w).reshape(x_hat.shape).contiguous()
            # the residual is zero: only gram is used, and it is valid at info 1 (engine.WeightedGaussNewtonResult)
            gram = E.weighted_gauss_newton_step(T, w, x_hat, x_hat, torch.zeros(Bc, dtype=torch.float64, device=dev), d=d).gram
            n_obs = (w > 0).flatten(1).sum(1)
        elif a is not None:
            if wrapper is None:
                K = E.operator_apply(T, a, x_hat)[0]
            else:
                K, _, scale = E.operator_apply_wrapped(T, a, x_hat, wrapper[:3])
            gram = E.gram_cholesky(K, d, 1).jtj
            n_obs = torch.full((Bc,), a.shape[0], dtype=torch.int64, device=dev)
        else:
            gram = E.gram_cholesky(T, d, 1).jtj
            n_obs = torch.full((Bc,), T.N, dtype=torch.int64, device=dev)
        r = E.tangent_leverage(T, gram)                               # on the sweep's J, whatever the normal matrix came from
        sigma2, dof = noise_level(n_obs, d, cost, variance)
        cov = sigma2[:, None, None] * r.cov
        std_head = (sigma2[:, None] * r.lev).sqrt().float()
        out = {"latent_covariance": cov, "latent_std": torch.diagonal(cov, dim1=1, dim2=2).sqrt(),
               "reconstruction_std_head": std_head.view(x_hat.shape), "leverage": r.lev.view(x_hat.shape),
               "noise_variance": sigma2, "dof": dof, "info": r.info}
        if wrapper is not None:
            s = scale.abs() if scale is not None else wrapper_derivative(wrapper[:3], x_hat)
            std = std_head * s.view(Bc, -1)
            if wrapper[3] is not None:                                # head element r is data element perm[r]
                std = torch.empty_like(std).index_copy_(1, wrapper[3].to(dev), std)
            out["reconstruction_std"] = std.view(Bc, *data_shape)
        return out
