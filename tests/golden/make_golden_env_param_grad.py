#!/usr/bin/env python3
"""Generate tests/golden/env_param_grad_f64.npz: the parameter gradient of the simulator linearisation, from the
unmodified reference's own PendulumDx / CartpoleDx modules (mpc/env_dx/pendulum.py:49-84, cartpole.py:63-96).

For each of the three simulators: N = 40 random points (x, u) -- unit-circle and off-circle (cos, sin) pairs, about a
fifth of the controls outside the module's clamp, two exactly on it --, non-default parameters, random cotangents
(gF, gf), and in float64

    F = d module(x, u) / d [x; u]      (n_state autograd passes, create_graph=True, as MPC.linearize_dynamics does)
    f = module(x, u) - F [x; u]
    gparams = d ( sum(gF * F) + sum(gf * f) ) / d params          (x, u detached leaves, mpc/mpc.py:495-497)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_env_param_grad.py

Needs the reference checkout make_golden.py reads; nothing at test time does."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden  # noqa: E402

SEED = 81
N = 40
CASES = (("pendulum", "pendulum", True, (9.5, 1.1, 0.9)),
         ("pendulum_full", "pendulum", False, (10., 1., 1., 0.3, 0.2)),
         ("cartpole", "cartpole", True, (9.8, 1.2, 0.15, 0.6)))


def points(kind, umax, g):
    f64 = torch.float64
    th = (torch.rand(N, generator=g, dtype=f64) - 0.5) * 2 * np.pi
    r = 1.0 + 0.1 * torch.randn(N, generator=g, dtype=f64)
    r[: N // 2] = 1.0                                                   # half of the points on the unit circle
    w = 2.0 * torch.randn(N, generator=g, dtype=f64)
    if kind == "pendulum":
        x = torch.stack((r * th.cos(), r * th.sin(), w), 1)
    else:
        z = torch.randn(N, 2, generator=g, dtype=f64)
        x = torch.stack((z[:, 0], z[:, 1], r * th.cos(), r * th.sin(), w), 1)
    u = (torch.rand(N, 1, generator=g, dtype=f64) - 0.5) * 2.5 * umax   # |u| up to 1.25 u_max: a fifth outside the clamp
    u[0, 0], u[1, 0] = umax, -umax                                      # the closed ends of the clamp
    return x, u


def case(kind, simple, params, g):
    prm = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    dx = make_golden._ref_env(kind, simple, prm)
    dx.params = prm
    ns = dx.n_state
    umax = dx.upper
    x, u = points(kind, umax, g)
    gF = torch.randn(N, ns, ns + 1, generator=g, dtype=torch.float64)
    gf = torch.randn(N, ns, generator=g, dtype=torch.float64)
    xt, ut = x.clone().requires_grad_(True), u.clone().requires_grad_(True)
    new_x = dx(xt, ut)
    rows = [torch.autograd.grad(new_x[:, j].sum(), [xt, ut], retain_graph=True, create_graph=True) for j in range(ns)]
    R, S = torch.stack([r[0] for r in rows], 1), torch.stack([r[1] for r in rows], 1)
    F = torch.cat((R, S), 2)
    f = new_x - (R * xt.unsqueeze(1)).sum(2) - (S * ut.unsqueeze(1)).sum(2)
    gparams, = torch.autograd.grad((gF * F).sum() + (gf * f).sum(), prm)
    n_out = int((u.abs() > umax).sum())
    return dict(x=x, u=u, params=prm, gF=gF, gf=gf, F=F, f=f, gparams=gparams, u_max=torch.tensor([umax], dtype=torch.float64),
                dt=torch.tensor([dx.dt], dtype=torch.float64), n_outside_clamp=torch.tensor([n_out]))


if __name__ == "__main__":
    g = torch.Generator().manual_seed(SEED)
    out = {}
    for name, kind, simple, params in CASES:
        c = case(kind, simple, params, g)
        print("%-14s outside the clamp: %d of %d   gparams %s" % (name, int(c["n_outside_clamp"]), N, make_golden.npy(c["gparams"])))
        for k, v in c.items():
            out[name + "_" + k] = make_golden.npy(v)
    make_golden.save("env_param_grad_f64", **out)
