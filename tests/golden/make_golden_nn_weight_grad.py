#!/usr/bin/env python3
"""Generate tests/golden/nn_weight_grad_f64.npz: the weight gradient of the NNDynamics linearisation, from the unmodified
reference's own NNDynamics module (mpc/dynamics.py:15-128).

For each network -- (5, 2, [20]) sigmoid and relu, (6, 3, [40, 24]) sigmoid, (12, 4, [100]) relu without passthrough,
(3, 1, []) -- in float64, with stored weights: random points (x, u), random cotangents (gF, gf) and

    F = [R | S],  (R, S) = module.grad_input(x, u) after module(x, u)       (mpc/mpc.py:495-503)
    f = module(x, u) - F [x; u]
    g = d ( sum(gF * F) + sum(gf * f) ) / d (every weight and bias)          (x, u detached leaves, mpc/mpc.py:495-497)

Weights, points and cotangents are rounded to float32 before use (stored as float64: the float32 kernels run the fixture
at exactly these numbers); relu points with a hidden pre-activation |h| < 1e-3 are redrawn.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nn_weight_grad.py

Needs the reference checkout make_golden.py reads; nothing at test time does."""
import os
import sys

import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden  # noqa: E402

SEED = 101
CASES = (("s5", 5, 2, [20], "sigmoid", True, 12),
         ("r5", 5, 2, [20], "relu", True, 12),
         ("s6", 6, 3, [40, 24], "sigmoid", True, 12),
         ("r12", 12, 4, [100], "relu", False, 8),
         ("lin3", 3, 1, [], "sigmoid", True, 12))


def r32(t):
    return t.to(torch.float32).to(torch.float64)


def case(ns, nc, hidden, act, passthrough, N, g):
    from mpc_ref.dynamics import NNDynamics
    f64 = torch.float64
    dyn = NNDynamics(ns, nc, list(hidden), activation=act, passthrough=passthrough).double()
    with torch.no_grad():
        for fc in dyn.fcs:
            fc.weight.copy_(r32(fc.weight))
            fc.bias.copy_(r32(fc.bias))
    n = ns + nc
    pts = []
    while len(pts) < N:
        tau = r32(torch.randn(n, generator=g, dtype=f64))
        a, ok = tau, True
        with torch.no_grad():
            for fc in list(dyn.fcs)[:-1]:
                h = fc(a)
                ok = ok and (act != "relu" or bool((h.abs() >= 1e-3).all()))
                a = torch.sigmoid(h) if act == "sigmoid" else torch.relu(h)
        if ok:
            pts.append(tau)
    tau = torch.stack(pts)
    x, u = tau[:, :ns].clone(), tau[:, ns:].clone()
    gF = r32(torch.randn(N, ns, n, generator=g, dtype=f64))
    gf = r32(torch.randn(N, ns, generator=g, dtype=f64))
    xt, ut = x.clone().requires_grad_(True), u.clone().requires_grad_(True)
    new_x = dyn(xt, ut)
    R, S = dyn.grad_input(xt, ut)
    F = torch.cat((R, S), 2)
    f = new_x - (R * xt.unsqueeze(1)).sum(2) - (S * ut.unsqueeze(1)).sum(2)
    params = [t for fc in dyn.fcs for t in (fc.weight, fc.bias)]
    grads = torch.autograd.grad((gF * F).sum() + (gf * f).sum(), params)
    out = dict(x=x, u=u, gF=gF, gf=gf, F=F, f=f, passthrough=torch.tensor([int(passthrough)]),
               act=torch.tensor([0 if act == "sigmoid" else 1]))
    for l, fc in enumerate(dyn.fcs):
        out["W%d" % l], out["b%d" % l] = fc.weight, fc.bias
        out["gW%d" % l], out["gb%d" % l] = grads[2 * l], grads[2 * l + 1]
    return out


if __name__ == "__main__":
    torch.manual_seed(SEED)
    g = torch.Generator().manual_seed(SEED)
    out = {}
    for name, ns, nc, hidden, act, passthrough, N in CASES:
        c = case(ns, nc, hidden, act, passthrough, N, g)
        print("%-5s %d points, |gW0| max %.3g" % (name, N, float(c["gW0"].abs().max())))
        for k, v in c.items():
            out[name + "_" + k] = make_golden.npy(v)
    make_golden.save("nn_weight_grad_f64", **out)
