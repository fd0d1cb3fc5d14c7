#!/usr/bin/env python3
"""Timings of the differentiable NNDynamics linearisation on the GPU box, for cotangents (gF, gf) of (F, f):

  (a) _native.MlpLinearizeFn forward + backward: mpc_mlp_linearize + mpc_mlp_param_grad
  (b) the route it replaces: MPC.linearize_dynamics(ANALYTIC, diff=True) through the module in torch (forward + grad_input
      with [N, hidden, n] intermediates) + torch.autograd.grad of the same contraction -- same process, same inputs
  (c) mpc_mlp_linearize alone, the floor
  (d) mpc_mlp_param_grad alone (HipBackend.mlp_linearize_backward)

Device events around windows of `reps` calls in the sustained state, the routes alternating, `rounds` windows each; the
record holds every window and the median.
usage: python tools/nn_param_grad_bench.py [ns nc hidden B T]     (defaults 12 4 100 4096 50; hidden: 100 or 40,24)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc.pytorch_amd"))
sys.path.insert(0, ROOT)


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
    from mpc.dynamics import NNDynamics
    arg = sys.argv[1:]
    ns, nc = (int(arg[0]), int(arg[1])) if len(arg) > 1 else (12, 4)
    hidden = [int(h) for h in arg[2].split(",") if h] if len(arg) > 2 else [100]
    B = int(arg[3]) if len(arg) > 3 else 4096
    T = int(arg[4]) if len(arg) > 4 else 50
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = "cuda:0"
    be = _native.backend()
    torch.manual_seed(1)
    dx = NNDynamics(ns, nc, hidden, activation="sigmoid").to(dev)
    plain = NNDynamics(ns, nc, hidden, activation="sigmoid").to(dev)
    plain.load_state_dict(dx.state_dict())
    plain.native_net = lambda like: None          # the module as the commit before the kernel route saw a diff=True call
    g = torch.Generator().manual_seed(1)
    N, n = (T - 1) * B, ns + nc
    x = torch.randn(T, B, ns, generator=g).to(dev)
    u = torch.randn(T, B, nc, generator=g).to(dev)
    gF = torch.randn(T - 1, B, ns, n, generator=g).to(dev)
    gf = torch.randn(T - 1, B, ns, generator=g).to(dev)
    ctrl = mpc.MPC(ns, nc, T, grad_method=mpc.GradMethods.ANALYTIC, weight_grad_kernel=True)
    X, U = x[:-1].reshape(-1, ns), u[:-1].reshape(-1, nc)
    net = dx.native_net(x)
    assert net is not None and net.param_grad_supported() and ctrl._param_grad_net(dx, x) is not None
    assert ctrl._param_grad_net(plain, x) is None

    def route(d):
        F, f = ctrl.linearize_dynamics(x, u, d, diff=True)
        return torch.autograd.grad((F * gF).sum() + (f * gf).sum(), list(d.fcs.parameters()))
    fns = {"a_function_fwd_bwd": lambda: route(dx), "b_module_autograd": lambda: route(plain),
           "c_mlp_linearize": lambda: be.mlp_linearize(net, X, U),
           "d_mlp_param_grad": lambda: be.mlp_linearize_backward(net, X, U, gF.view(N, ns, n), gf.view(N, ns))}
    ga, gb = route(dx), route(plain)
    torch.cuda.synchronize()
    res = {"ns": ns, "nc": nc, "hidden": hidden, "B": B, "T": T, "N": N, "device": torch.cuda.get_device_name(0),
           "grad_max_diff_over_max": [float((a - b).abs().max() / b.abs().max()) for a, b in zip(ga, gb)]}
    reps = {"a_function_fwd_bwd": 20, "b_module_autograd": 5, "c_mlp_linearize": 40, "d_mlp_param_grad": 20}
    rounds = 5
    for name, fn in fns.items():         # warm up every route at this shape
        window_ms(fn, max(2, reps[name] // 5))
    windows = {name: [] for name in fns}
    for _ in range(rounds):              # the routes alternate
        for name, fn in fns.items():
            windows[name].append(window_ms(fn, reps[name]))
    for name, w in windows.items():
        res[name + "_ms"] = {"median": statistics.median(w), "min": min(w), "max": max(w), "windows": w, "calls_per_window": reps[name]}
    res["b_over_a"] = res["b_module_autograd_ms"]["median"] / res["a_function_fwd_bwd_ms"]["median"]
    print(json.dumps({k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median", "min", "max")}) for k, v in res.items()}))
    out_dir = os.environ.get("MPC_BENCH_RECORD_DIR") or os.path.join(ROOT, "bench_records")
    os.makedirs(out_dir, exist_ok=True)
    name = "nn_param_grad_bench_%d_%d_%s_B%d_T%d.json" % (ns, nc, "x".join(map(str, hidden)), B, T)
    json.dump(res, open(os.path.join(out_dir, name), "w"), indent=1)


if __name__ == "__main__":
    main()
