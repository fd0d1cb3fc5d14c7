#!/usr/bin/env python3
"""Recover a simulator's physical parameters through the controller: a pendulum with perturbed (g, m, l) is trained so
that MPC on IT reproduces the controls an expert computes on the true pendulum -- the loss is on the controller's
output, the gradient reaches the three parameters through the KKT backward of the LQR step and the backward of the
simulator's linearisation.

Every MPC.forward here runs the simulator inside the kernels (trajectory, closed-form linearisation, line-searched
rollout); the last, differentiable linearisation of a solve is a kernel as well (mpc_env_linearize forward,
mpc_env_param_grad backward: _native.EnvLinearizeFn), so a training step never leaves the device.

    python examples/learn_simulator_params.py [n_batch] [epochs]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mpc.pytorch_amd"))
from mpc import mpc                                    # noqa: E402
from mpc.mpc import QuadCost, GradMethods              # noqa: E402
from mpc.env_dx import pendulum                        # noqa: E402

dev = "cuda:0"
n_batch = int(sys.argv[1]) if len(sys.argv) > 1 else 128
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 200
T = 10
torch.manual_seed(0)
true_dx = pendulum.PendulumDx()
q, p = true_dx.get_true_obj()
Q = torch.diag(q).repeat(T, n_batch, 1, 1).to(dev)
pp = p.repeat(T, n_batch, 1).to(dev)
cost = QuadCost(Q, pp)


def controller(lqr_iter=15):
    return mpc.MPC(true_dx.n_state, true_dx.n_ctrl, T, u_lower=true_dx.lower, u_upper=true_dx.upper, lqr_iter=lqr_iter,
                   verbose=-1, exit_unconverged=False, detach_unconverged=False, grad_method=GradMethods.AUTO_DIFF,
                   linesearch_decay=true_dx.linesearch_decay, max_linesearch_iter=true_dx.max_linesearch_iter)


def sample_states(n):
    th = (torch.rand(n) - 0.5) * 2.0
    return torch.stack((th.cos(), th.sin(), (torch.rand(n) - 0.5)), 1).to(dev)


# the learner starts 20-30 % off; its parameters live on the host, where the optimiser works on them
params = torch.tensor((8.0, 1.3, 0.8), requires_grad=True)
learner = pendulum.PendulumDx(params=params)
opt = torch.optim.Adam([params], lr=2e-2)
t0 = time.time()
for epoch in range(epochs):
    x0 = sample_states(n_batch)
    with torch.no_grad():
        _, u_expert, _ = controller()(x0, cost, true_dx)
    _, u_learner, _ = controller()(x0, cost, learner)
    loss = (u_learner - u_expert).pow(2).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    if epoch % 20 == 0 or epoch + 1 == epochs:
        g, m, l = params.tolist()
        # (the controls see the parameters through g / l and m l^2 only: those two are what imitation can recover)
        print("epoch %3d  imitation loss %.6f   g/l %.3f (true %.1f)   m l^2 %.3f (true %.1f)   (%.1f s)"
              % (epoch, float(loss.detach()), g / l, 10.0, m * l * l, 1.0, time.time() - t0))
print("done: %d solves of %d problems each" % (2 * epochs, n_batch))
