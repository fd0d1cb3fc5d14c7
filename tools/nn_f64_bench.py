#!/usr/bin/env python3
"""Timings of no-grad float64 solves through an NNDynamics on the GPU box: the `network` route on the float64 kernels
(csrc/nn_dynamics64.hip: linearise, generic float64 sweep, rollout -- three C calls an iteration) against the module path in the
same process, which is what a float64 network took before those kernels existed (`_iterate_general`: the module called from
Python once per timestep and trial, [N, hidden, n] intermediates in the linearisation).  The module path is the same network as a
subclass that overrides `forward` by calling `super()`: `native_net` declines it.

Rows (5 iterations, eps = 0, sigmoid, hidden [100]):
  nn12       NNDynamics(12, 4, [100]), T = 50, B = 1024, unbounded
  nn12_box   the same with u in [-1, 1]
  nn32       NNDynamics(32, 8, [100]), T = 64, B = 1024, unbounded
  nn32_box   the same with u in [-1, 1]

The two routes alternate in one process after a run-up solve of each.  A window of the kernel route is as many solves as fill
`--window-ms` (measured once after the run-up), a window of the module route one solve (hundreds of milliseconds); a window is
timed on the host clock from the first call to a device synchronise behind the last (MPC.forward reads its convergence flags
back, so host time is part of a solve).  Reported per solve: median (min - max) of `--rounds` windows.
Also timed alone, with device events around `--call-reps` back-to-back calls on the solve's first nominal: the three calls of one
iteration -- HipBackend.mlp_linearize, lqr_step(sweep_only), mlp_rollout.
usage: python tools/nn_f64_bench.py [--rows nn12,nn12_box,nn32,nn32_box] [--rounds 7] [--window-ms 300]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc.pytorch_amd"))
sys.path.insert(0, ROOT)

SHAPES = {"nn12": (12, 4, 50, 1024), "nn32": (32, 8, 64, 1024)}


def make_row(row, dev):
    from mpc import mpc
    from mpc.dynamics import NNDynamics
    from mpc.mpc import QuadCost

    class ModulePath(NNDynamics):
        def forward(self, x, u):
            return super().forward(x, u)
    ns, nc, T, B = SHAPES[row.split("_")[0]]
    n = ns + nc
    box = row.endswith("_box")
    torch.manual_seed(3)
    plain = NNDynamics(ns, nc, [100], activation="sigmoid").double().to(dev)
    module = ModulePath(ns, nc, [100], activation="sigmoid").double().to(dev)
    module.load_state_dict(plain.state_dict())
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    L = r(T, B, n, n)
    C = (L @ L.transpose(2, 3) / n + torch.eye(n, dtype=torch.float64)).to(dev)
    c = r(T, B, n).to(dev)
    x0 = r(B, ns).to(dev)
    kw = dict(u_lower=-1.0, u_upper=1.0) if box else {}

    def make():
        return mpc.MPC(ns, nc, T, lqr_iter=5, verbose=-1, exit_unconverged=False, detach_unconverged=False, backprop=False, eps=0.0,
                       grad_method=mpc.GradMethods.ANALYTIC, **kw)
    meta = dict(n_state=ns, n_ctrl=nc, hidden=[100], T=T, B=B, lqr_iter=5, dtype="float64", box=box)
    return make, x0, QuadCost(C, c), plain, module, meta, kw


def window_ms(ctrl, args, solves):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for _ in range(solves):
            out = ctrl(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / solves, out


def summary(w):
    return {"median": statistics.median(w), "min": min(w), "max": max(w), "repeats": w}


def iteration_calls(x0, cost, plain, kw, reps):
    """Device time of each of the three calls of one iteration, at the zero-control nominal."""
    from mpc import _native
    from mpc._native import StepOptions
    be = _native.backend()
    T, B, n = cost.C.shape[0], cost.C.shape[1], cost.C.shape[2]
    ns = x0.shape[1]
    nc = n - ns
    net = plain.native_net(x0)
    u = torch.zeros(T, B, nc, device=x0.device, dtype=x0.dtype)
    x, _ = be.mlp_traj_cost(x0, u, net)
    px, pu = x[:-1].reshape(-1, ns), u[:-1].reshape(-1, nc)
    F, f = be.mlp_linearize(net, px, pu)
    F, f = F.view(T - 1, B, ns, n), f.view(T - 1, B, ns)
    opts = StepOptions(u_lower=kw.get("u_lower"), u_upper=kw.get("u_upper"))
    sweep = StepOptions(u_lower=kw.get("u_lower"), u_upper=kw.get("u_upper"), sweep_only=True)
    s = be.lqr_step(x0, cost.C, cost.c, F, f, x, u, sweep, want_gains=True)
    calls = {
        "linearize_ms": lambda: be.mlp_linearize(net, px, pu),
        "sweep_ms": lambda: be.lqr_step(x0, cost.C, cost.c, F, f, x, u, sweep, want_gains=True),
        "rollout_ms": lambda: be.mlp_rollout(x0, cost.C, cost.c, s["K"], s["k"], x, u, s["old_costs"], opts, net),
    }
    res = {}
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        res[name] = a.elapsed_time(b) / reps
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="nn12,nn12_box,nn32,nn32_box")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--call-reps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "rows": {}}
    for row in a.rows.split(","):
        make, x0, cost, plain, module, meta, kw = make_row(row, dev)
        on, off = make(), make()
        assert on.solve_route(x0, cost, plain).loop == "network", "the float64 kernels must take this network"
        assert off.solve_route(x0, cost, module).loop == "general"
        t_on, o_on = window_ms(on, (x0, cost, plain), 1)               # run-up of either route at this shape
        _, o_off = window_ms(off, (x0, cost, module), 1)
        t_on, _ = window_ms(on, (x0, cost, plain), 3)
        solves = max(1, int(round(a.window_ms / t_on)))
        w_on, w_off = [], []
        for _ in range(a.rounds):                                        # the routes alternate
            w_on.append(window_ms(on, (x0, cost, plain), solves)[0])
            w_off.append(window_ms(off, (x0, cost, module), 1)[0])
        rec = dict(meta, solves_per_kernel_window=solves, kernel_route_ms=summary(w_on), module_route_ms=summary(w_off))
        rec["module_over_kernel"] = rec["module_route_ms"]["median"] / rec["kernel_route_ms"]["median"]
        rec["max_abs_du_between_routes"] = float((o_on[1] - o_off[1]).abs().max())
        rec["mean_cost_kernel"], rec["mean_cost_module"] = float(o_on[2].mean()), float(o_off[2].mean())
        rec["one_iteration"] = iteration_calls(x0, cost, plain, kw, a.call_reps)
        res["rows"][row] = rec
        print(json.dumps({row: {k: (v if not (isinstance(v, dict) and "repeats" in v) else {q: v[q] for q in ("median", "min", "max")})
                                for k, v in rec.items()}}), flush=True)
    out_dir = os.environ.get("MPC_BENCH_RECORD_DIR") or os.path.join(ROOT, "bench_records")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "nn_f64_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
