#!/usr/bin/env python3
"""Timings of the differentiable simulator linearisation on the GPU box, for cotangents (gF, gf) of (F, f):

  (a) _native.EnvLinearizeFn forward + backward: mpc_env_linearize + mpc_env_param_grad
  (b) the route it replaces: MPC.linearize_dynamics(diff=True) through the module in torch (n_state backward passes with
      create_graph=True) + torch.autograd.grad of the same contraction -- same process, same inputs
  (c) mpc_env_linearize alone, the floor
  (d) mpc_env_param_grad alone (HipBackend.env_linearize_backward)

Device events around windows of `reps` calls in the sustained state, the routes alternating, `rounds` windows each; the
record holds every window and the median.
usage: python tools/env_param_grad_bench.py [kind] [B] [T] [dtype]     (defaults pendulum 1024 20 float32;
                                                                       kind: pendulum | pendulum_full | cartpole)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc.pytorch_amd"))
sys.path.insert(0, ROOT)

PARAMS = {"pendulum": (10., 1., 1.), "pendulum_full": (10., 1., 1., 0.3, 0.2), "cartpole": (9.8, 1.0, 0.1, 0.5)}


def window_ms(fn, reps):
    """milliseconds per call over one window of `reps` calls, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    from mpc import _native, mpc
    from mpc.env_dx import cartpole, pendulum
    kind = sys.argv[1] if len(sys.argv) > 1 else "pendulum"
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    dtype = getattr(torch, sys.argv[4]) if len(sys.argv) > 4 else torch.float32
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = "cuda:0"
    be = _native.backend()

    def make(hide):
        prm = torch.tensor(PARAMS[kind], dtype=dtype, device=dev, requires_grad=True)
        dx = cartpole.CartpoleDx(params=prm) if kind == "cartpole" else pendulum.PendulumDx(params=prm, simple=(kind == "pendulum"))
        if hide:                     # the module as the commit before the kernel route saw it
            dx.__class__ = type("Plain" + type(dx).__name__, (type(dx),), {"native_param_grad": None})
        return dx, prm
    dx, prm = make(False)
    plain, prm_b = make(True)
    ns = dx.n_state
    g = torch.Generator().manual_seed(1)
    th = (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * 2.0
    zero = torch.zeros(B, dtype=torch.float64)
    x0 = (torch.stack((zero, zero, th.cos(), th.sin(), zero), 1) if kind == "cartpole" else torch.stack((th.cos(), th.sin(), zero), 1))
    x0 = x0.to(dtype).to(dev)
    u = ((torch.rand(T, B, 1, generator=g, dtype=torch.float64) - 0.5) * 2.5 * dx.upper * (0.05 if kind == "cartpole" else 1.0)).to(dtype).to(dev)
    x, _ = be.env_traj_cost(x0, u, dx.native_env())
    N = (T - 1) * B
    gF = torch.randn(T - 1, B, ns, ns + 1, generator=g, dtype=torch.float64).to(dtype).to(dev)
    gf = torch.randn(T - 1, B, ns, generator=g, dtype=torch.float64).to(dtype).to(dev)
    ctrl = mpc.MPC(ns, 1, T, grad_method=mpc.GradMethods.AUTO_DIFF)
    X, U = x[:-1].reshape(-1, ns), u[:-1].reshape(-1, 1)
    env = dx.native_env()

    def route(d, p):
        F, f = ctrl.linearize_dynamics(x, u, d, diff=True)
        return torch.autograd.grad((F * gF).sum() + (f * gf).sum(), p)[0]
    fns = {"a_function_fwd_bwd": lambda: route(dx, prm), "b_module_autograd": lambda: route(plain, prm_b),
           "c_env_linearize": lambda: be.env_linearize(env, X, U),
           "d_env_param_grad": lambda: be.env_linearize_backward(env, X, U, gF.view(N, ns, ns + 1), gf.view(N, ns))}
    ga, gb = route(dx, prm), route(plain, prm_b)
    torch.cuda.synchronize()
    res = {"kind": kind, "B": B, "T": T, "N": N, "dtype": str(dtype), "device": torch.cuda.get_device_name(0),
           "grad_function": ga.tolist(), "grad_module": gb.tolist(),
           "grad_rel_diff": float(((ga - gb).abs() / (gb.abs() + 1e-30)).max())}
    reps = {"a_function_fwd_bwd": 200, "b_module_autograd": 20, "c_env_linearize": 400, "d_env_param_grad": 400}
    rounds = 7
    for name, fn in fns.items():         # warm up every route at this shape
        window_ms(fn, max(3, reps[name] // 10))
    windows = {name: [] for name in fns}
    for _ in range(rounds):              # the routes alternate
        for name, fn in fns.items():
            windows[name].append(window_ms(fn, reps[name]))
    for name, w in windows.items():
        res[name + "_ms"] = {"median": statistics.median(w), "min": min(w), "max": max(w), "windows": w, "calls_per_window": reps[name]}
    res["b_over_a"] = res["b_module_autograd_ms"]["median"] / res["a_function_fwd_bwd_ms"]["median"]
    print(json.dumps({k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median", "min", "max")}) for k, v in res.items()}, indent=1))
    out_dir = os.environ.get("MPC_BENCH_RECORD_DIR") or os.path.join(ROOT, "bench_records")
    os.makedirs(out_dir, exist_ok=True)
    name = "env_param_grad_bench_%s_B%d_T%d_%s.json" % (kind, B, T, str(dtype).split(".")[-1])
    json.dump(res, open(os.path.join(out_dir, name), "w"), indent=1)


if __name__ == "__main__":
    main()
