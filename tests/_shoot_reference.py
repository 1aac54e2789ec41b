"""The shooting loop of ``cmf_amd.ManifoldGeodesic.shoot_latents`` on the oracle, in float64 (or float32, the
yardstick): Hamilton's equations z' = v = G^-1 p, p' = grad_z 1/2 ||J(z) v||^2 with v held fixed, classical RK4 with equal steps,
the node's own evaluation as the first stage, a closing evaluation for the speed at the last node, and the ``log`` velocity formula.
v is ``torch.linalg.solve(G, p)`` under ``no_grad``; p' is ``torch.autograd.grad`` through ``oracle.cmf_oracle.jvp_forward``.  The
host tests establish on it the conditions the GPU tests assert of the product."""
import copy

import torch

import _geodesic_reference as GR
from _projection_reference import Model
from conftest import golden_model, load_golden
from oracle import cmf_oracle as O

MLP = ["c1_sphere_d2", "c2a_power", "c2b_hepmass"]
FIXTURES = MLP + ["mini_mnist", "mini_cifar"]
STEPS = 8

_MODELS = {}


def model_of(name, dtype=torch.float64):
    """The fixture's ``Model`` (float64), or the same model with the float32 oracle's parameters and inputs."""
    if (name, dtype) not in _MODELS:
        m = _MODELS[(name, torch.float64)] = _MODELS.get((name, torch.float64)) or Model(name)
        if dtype != torch.float64:
            m = copy.copy(m)
            m.sd = golden_model(load_golden(name)[1], dtype)[4]
            m.y = m.y.to(dtype)
            _MODELS[(name, dtype)] = m
    return _MODELS[(name, dtype)]


def endpoints(model, name):
    """The curves of ``_geodesic_reference.endpoints``; ``mini_cifar``: the first sample to the second."""
    if name == "mini_cifar":
        return model.y[:1], model.y[1:2]
    return GR.endpoints(model, name)


def metric(model, z):
    with torch.no_grad():
        return model.jacobian(z)[0]


def hamiltonian(model, z, p):
    """H = 1/2 p^T G(z)^-1 p per sample."""
    with torch.no_grad():
        return 0.5 * (p * torch.linalg.solve(metric(model, z), p[:, :, None])[:, :, 0]).sum(1)


def evaluate(model, z, p, backward=True, scale=1.0):
    """(p', v, p^T v) at (z, p); ``scale`` multiplies all three (the per-evaluation bound applied coherently)."""
    with torch.no_grad():
        v = torch.linalg.solve(metric(model, z), p[:, :, None])[:, :, 0]
        s2 = (p * v).sum(1)
    dp = None
    if backward:
        zz = z.clone().requires_grad_(True)
        jv = O.jvp_forward(model.sd, model.flow_ops, model.base, zz, v)[1]
        dp = torch.autograd.grad(0.5 * (jv.flatten(1) ** 2).sum(), zz)[0] * scale
    return dp, v * scale, s2 * scale


def shoot(model, z0, v0, steps=STEPS, time=1.0, scale=1.0):
    """The loop from the latents ``z0`` with the velocities ``v0`` (B, d), in their dtype."""
    h = time / steps
    with torch.no_grad():
        p = torch.bmm(metric(model, z0), v0[:, :, None])[:, :, 0]
    z = z0.clone()
    dp, v, s2 = evaluate(model, z, p, scale=scale)
    nodes = [(z, v, p, s2)]
    for i in range(steps):
        kz, kp = [v], [dp]
        for a in (0.5, 0.5, 1.0):
            dpa, va, _ = evaluate(model, z + (a * h) * kz[-1], p + (a * h) * kp[-1], scale=scale)
            kz.append(va)
            kp.append(dpa)
        z = z + (h / 6.0) * (kz[0] + 2.0 * kz[1] + 2.0 * kz[2] + kz[3])
        p = p + (h / 6.0) * (kp[0] + 2.0 * kp[1] + 2.0 * kp[2] + kp[3])
        dp, v, s2 = evaluate(model, z, p, backward=i + 1 < steps, scale=scale)
        nodes.append((z, v, p, s2))
    latents, velocity, momentum, speed2 = (torch.stack(t, 1) for t in zip(*nodes))
    speed = speed2.sqrt()
    with torch.no_grad():
        path = model.decode(latents.flatten(0, 1)).reshape(len(z0), steps + 1, -1)
    return {"latents": latents, "velocity": velocity, "momentum": momentum, "speed2": speed2,
            "length": h * (0.5 * (speed[:, :-1] + speed[:, 1:])).sum(1), "path_head": path}


def log_velocity(latents):
    """N (-3 z_0 + 4 z_1 - z_2) / 2 of a relaxed curve (B, P, d)."""
    z = latents.double()
    return (z.shape[1] - 1) * (-3.0 * z[:, 0] + 4.0 * z[:, 1] - z[:, 2]) / 2.0


def ends(name, dtype=torch.float64):
    """(model in ``dtype``, z0, z1): the float64 encoder's latents of the fixture's curves, rounded to float32 -- values every
    arithmetic under test can start from exactly -- and held in ``dtype``."""
    model = model_of(name)
    y0, y1 = endpoints(model, name)
    with torch.no_grad():
        z0, z1 = model.encode(y0).float(), model.encode(y1).float()
    return model_of(name, dtype), z0.to(dtype), z1.to(dtype)


_LOGS = {}


def log_run(name):
    """(model, z0, z1, relaxed): ``_geodesic_reference.connect`` with points = 9, steps = 10 between the fixture's ends, once."""
    if name not in _LOGS:
        if name in GR.FIXTURES:                                          # the geodesic host tests relax the same curves
            model, _, relaxed = GR.reference_run(name)
        else:
            model, z0, z1 = ends(name)
            with torch.no_grad():
                relaxed = GR.connect(model, z0, z1)
        _LOGS[name] = (model, relaxed["latents"][:, 0], relaxed["latents"][:, -1], relaxed)
    return _LOGS[name]


_RUNS = {}


def chord_run(name, dtype=torch.float64, scale=1.0):
    """The S = 8, time 1 shoot along the straight chord z1 - z0 of the fixture's curves, computed once per (dtype, scale)."""
    key = (name, dtype, scale)
    if key not in _RUNS:
        model, z0, z1 = ends(name, dtype)
        _RUNS[key] = (model, z0, z1, shoot(model, z0, z1 - z0, scale=scale))
    return _RUNS[key]
