#!/usr/bin/env python3
"""Golden fixtures of slew-rate solves (`slew_rate_penalty` / `prev_ctrl`, mpc/mpc.py:113-116, 362-445) from the UNMODIFIED
reference: a QuadCost with affine dynamics (posed as a module, see AffineDx: the reference cannot roll a LinDx out under a
penalty), and with the reference's own PendulumDx / CartpoleDx.

Run where the reference is mounted (the GPU box has none):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_slew.py

All float64.  The reference is called once per problem (n_batch = 1) and the results are stacked: the per-problem semantics
the kernels implement (its batch-global pnqp / line-search loops couple the problems of a batch).  Every .npz holds the
inputs and the reference's outputs, so nothing at test time needs the reference.
"""
import contextlib
import importlib
import importlib.util
import io
import os
import sys
import warnings

import numpy as np
import torch

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/mpc"


def load_reference():
    spec = importlib.util.spec_from_file_location(
        "mpc_ref", os.path.join(REF, "__init__.py"), submodule_search_locations=[REF])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["mpc_ref"] = pkg
    spec.loader.exec_module(pkg)
    import mpc_ref.mpc as ref_mpc          # noqa
    import mpc_ref.util as ref_util        # noqa
    sys.modules.setdefault("mpc", pkg)     # env_dx does `from mpc import util`
    sys.modules.setdefault("mpc.util", ref_util)
    return ref_mpc


ref_mpc = load_reference()
QuadCost, LinDx = ref_mpc.QuadCost, ref_mpc.LinDx


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def npy(t):
    return t.detach().cpu().numpy()


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    print("%-28s %6.1f KiB" % (name, os.path.getsize(path) / 1024.0))


def per_problem(make_ctrl, x_init, C, c, dyn_of, prev):
    """The reference once per problem; prev: None or a float (prev_ctrl = that value for every control)."""
    xs, us, cs = [], [], []
    for b in range(x_init.shape[0]):
        ctrl = make_ctrl(None if prev is None else torch.full((1, C.shape[2] - x_init.shape[1]), prev, dtype=torch.float64))
        x, u, costs = quiet(ctrl, x_init[b:b + 1], QuadCost(C[:, b:b + 1], c[:, b:b + 1]), dyn_of(b))
        xs.append(npy(x)); us.append(npy(u)); cs.append(npy(costs))
    return np.concatenate(xs, 1), np.concatenate(us, 1), np.concatenate(cs, 0)


class AffineDx(torch.nn.Module):
    """x+ = F [x;u] + f as a module with grad_input.  The reference cannot roll a LinDx out under a slew-rate penalty (its
    augmented `true_dynamics` is None there, mpc/mpc.py:412-415, and mpc/lqr_step.py:223-225 calls it), so the LinDx case is
    posed to it as this time-invariant module under GradMethods.ANALYTIC: the same problem, (F, f) repeated over t."""

    def __init__(self, F, f):
        super().__init__()
        self.F, self.f = F, f

    def forward(self, x, u):
        return torch.cat((x, u), 1) @ self.F.t() + self.f

    def grad_input(self, x, u):
        ns = self.F.shape[0]
        R = self.F[:, :ns].unsqueeze(0).repeat(x.shape[0], 1, 1)
        S = self.F[:, ns:].unsqueeze(0).repeat(x.shape[0], 1, 1)
        return R, S


def lin_case(name, seed, ns=3, nc=2, T=5, B=3, bound=0.5, gamma=1.0, lqr_iter=20):
    g = torch.Generator().manual_seed(seed)
    n = ns + nc
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    L = r(T, B, n, n)
    C = L @ L.transpose(2, 3) + 0.5 * torch.eye(n, dtype=torch.float64)
    c = r(T, B, n)
    F1 = 0.3 * r(B, ns, n) + torch.cat((torch.eye(ns, dtype=torch.float64), torch.zeros(ns, nc, dtype=torch.float64)), 1)
    f1 = 0.1 * r(B, ns)
    F, f = F1.unsqueeze(0).repeat(T - 1, 1, 1, 1), f1.unsqueeze(0).repeat(T - 1, 1, 1)
    x_init = r(B, ns)

    def make(prev):
        return ref_mpc.MPC(ns, nc, T, u_lower=-bound, u_upper=bound, lqr_iter=lqr_iter, verbose=-1, exit_unconverged=False,
                           detach_unconverged=False, backprop=False, grad_method=ref_mpc.GradMethods.ANALYTIC,
                           slew_rate_penalty=gamma, prev_ctrl=prev)
    x, u, costs = per_problem(make, x_init, C, c, lambda b: AffineDx(F1[b], f1[b]), None)
    save(name, meta=np.array([ns, nc, T, B, lqr_iter]), gamma=np.array([gamma]), bound=np.array([bound]),
         x_init=npy(x_init), C=npy(C), c=npy(c), F=npy(F), f=npy(f), x=x, u=u, costs=costs)
    print("   controls on a bound: %d of %d" % (int((np.abs(np.abs(u) - bound) < 1e-9).sum()), u.size))


def env_case(name, kind, seed, T=8, B=4, lqr_iter=8):
    """make_golden.py's env_case recipe with a slew-rate penalty: gamma = 0.5 without prev_ctrl, gamma = 2 with prev_ctrl = 0.3."""
    mod = importlib.import_module("mpc_ref.env_dx." + kind)
    dx = getattr(mod, "PendulumDx" if kind == "pendulum" else "CartpoleDx")()
    dx.params = dx.params.double()
    ns, nc = dx.n_state, dx.n_ctrl
    g = torch.Generator().manual_seed(seed)
    if kind == "pendulum":
        th = (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * np.pi
        thd = (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * 2.0
        x_init = torch.stack((torch.cos(th), torch.sin(th), thd), 1)
    else:
        th = (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * 0.6
        z = 0.2 * torch.randn(B, 3, generator=g, dtype=torch.float64)
        x_init = torch.stack((z[:, 0], z[:, 1], torch.cos(th), torch.sin(th), z[:, 2]), 1)
    q, p_ = dx.get_true_obj()
    q, p_ = q.double(), p_.double()
    Q = torch.diag(q).unsqueeze(0).unsqueeze(0).repeat(T, B, 1, 1)
    pp = p_.unsqueeze(0).repeat(T, B, 1)
    out = {}
    for tag, gamma, prev in (("a", 0.5, None), ("b", 2.0, 0.3)):
        def make(prev_t, gamma=gamma):
            return ref_mpc.MPC(ns, nc, T, u_lower=dx.lower, u_upper=dx.upper, lqr_iter=lqr_iter, verbose=-1,
                               exit_unconverged=False, detach_unconverged=False, backprop=False,
                               linesearch_decay=dx.linesearch_decay, max_linesearch_iter=dx.max_linesearch_iter,
                               grad_method=ref_mpc.GradMethods.AUTO_DIFF, eps=dx.mpc_eps, slew_rate_penalty=gamma,
                               prev_ctrl=prev_t)
        x, u, costs = per_problem(make, x_init, Q, pp, lambda b: dx, prev)
        out.update({"gamma_" + tag: np.array([gamma]), "prev_" + tag: np.array([0.0 if prev is None else prev]),
                    "has_prev_" + tag: np.array([prev is not None]), "x_" + tag: x, "u_" + tag: u, "costs_" + tag: costs})
        print("   %s: controls on a bound: %d of %d" % (tag, int((np.abs(np.abs(u) - dx.upper) < 1e-9).sum()), u.size))
    save(name, meta=np.array([ns, nc, T, B, lqr_iter]), x_init=npy(x_init), Q=npy(Q), p=npy(pp), params=npy(dx.params),
         lower=np.array([dx.lower]), upper=np.array([dx.upper]), decay=np.array([dx.linesearch_decay]),
         max_ls=np.array([dx.max_linesearch_iter]), eps=np.array([dx.mpc_eps]), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    lin_case("mpc_slew_lin_f64", 21)
    env_case("mpc_slew_pendulum_f64", "pendulum", 51)
    env_case("mpc_slew_cartpole_f64", "cartpole", 52)
