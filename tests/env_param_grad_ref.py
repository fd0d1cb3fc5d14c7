"""Shared by tests/test_env_param_grad.py and tests/test_gpu_env_param_grad.py: the float64 yardstick of the simulator
linearisation's parameter gradient -- torch autograd through the package's own `_transition` (which
tests/test_host_logic.py pins to the reference's modules), with create_graph=True, contracted with (gF, gf) -- and
the random points the kernel is run on."""
import numpy as np
import torch

KINDS = ("pendulum", "pendulum_full", "cartpole")
# non-default parameters (damping and gravity bias of the full pendulum included)
PARAMS = {"pendulum": (9.5, 1.1, 0.9), "pendulum_full": (10., 1., 1., 0.3, 0.2), "cartpole": (9.8, 1.2, 0.15, 0.6)}


def make_dx(kind, params):
    from mpc.env_dx import cartpole, pendulum
    if kind == "cartpole":
        return cartpole.CartpoleDx(params=params)
    return pendulum.PendulumDx(params=params, simple=(kind == "pendulum"))


def yardstick(kind, params, x, u, gF, gf):
    with torch.enable_grad():          # (also callable from inside an autograd backward, where grad mode is off)
        return _yardstick(kind, params, x, u, gF, gf)


def _yardstick(kind, params, x, u, gF, gf):
    """float64 (F, f, gparams, scale) at the points x [N,ns], u [N,1] for cotangents gF [N,ns,ns+1], gf [N,ns]:
    gparams_k = d (sum gF F + sum gf f) / d p_k with x, u constants; scale_k = sum over the points of |that point's
    contribution| (every point gets its own copy of the parameters: `_transition` unbinds them into [N] vectors)."""
    dev = x.device
    x, u, gF, gf = (t.detach().to(torch.float64) for t in (x, u, gF, gf))
    N = x.shape[0]
    prm = torch.as_tensor(params).detach().to(device=dev, dtype=torch.float64)
    dx = make_dx(kind, prm)
    P = prm.expand(N, prm.numel()).T.clone().requires_grad_(True)              # [np, N]
    xt, ut = x.clone().requires_grad_(True), u.clone().requires_grad_(True)
    new_x = dx._transition(xt, ut[:, 0].clamp(-dx._u_max, dx._u_max), P)
    ns = dx.n_state
    rows = [torch.autograd.grad(new_x[:, j].sum(), [xt, ut], retain_graph=True, create_graph=True) for j in range(ns)]
    R, S = torch.stack([r[0] for r in rows], 1), torch.stack([r[1] for r in rows], 1)
    F = torch.cat((R, S), 2)
    f = new_x - (R * xt.unsqueeze(1)).sum(2) - (S * ut.unsqueeze(1)).sum(2)
    per_point, = torch.autograd.grad((gF * F).sum() + (gf * f).sum(), P)
    return F.detach(), f.detach(), per_point.sum(1), per_point.abs().sum(1)


def random_points(kind, N, seed, device="cpu", dtype=torch.float64):
    """(x, u, gF, gf) in `dtype`: (cos, sin) on and off the unit circle, about 20 % of the controls outside the clamp and,
    from three points on, one exactly at +u_max and one at -u_max."""
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    u_max = make_dx(kind, torch.tensor(PARAMS[kind])).upper
    th = (torch.rand(N, generator=g, dtype=f64) - 0.5) * 2 * np.pi
    r = 1.0 + 0.1 * torch.randn(N, generator=g, dtype=f64)
    r[::2] = 1.0
    w = 2.0 * torch.randn(N, generator=g, dtype=f64)
    if kind == "cartpole":
        z = torch.randn(N, 2, generator=g, dtype=f64)
        x = torch.stack((z[:, 0], z[:, 1], r * th.cos(), r * th.sin(), w), 1)
    else:
        x = torch.stack((r * th.cos(), r * th.sin(), w), 1)
    u = (torch.rand(N, 1, generator=g, dtype=f64) - 0.5) * 2.5 * u_max
    if N >= 3:
        u[N // 3, 0], u[(2 * N) // 3, 0] = u_max, -u_max
    ns = x.shape[1]
    gF = torch.randn(N, ns, ns + 1, generator=g, dtype=f64)
    gf = torch.randn(N, ns, generator=g, dtype=f64)
    return tuple(t.to(dtype).to(device) for t in (x, u, gF, gf))
