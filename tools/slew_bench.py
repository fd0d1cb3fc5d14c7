#!/usr/bin/env python3
"""Timings of no-grad slew-rate solves (MPC.forward with slew_rate_penalty) on the GPU box: the device-side loop of round 11
(MPC._slew_plan fires) against the same solve with the predicate off -- `_iterate_general`, the behaviour of the commit before.

Rows:
  lin        12/4, T = 50, B = 4096, float32, 5 iterations, gamma = 1, unbounded (LinDx)
  lin_box    the same with u in [-1, 1]
  pendulum   PendulumDx, T = 20, B = 1024, 10 iterations, the module's own bounds and line search
  cartpole   CartpoleDx, T = 25, B = 4096, 10 iterations, the module's own bounds and line search
  nn         NNDynamics(12, 4, [100]), T = 50, B = 4096, float32, 5 iterations, gamma = 1, unbounded: `planned_network_slew=True`
             (the pre-bound network loop on the augmented problem, mpc_mlp_linearize_carry) against the flag off (`_iterate_general`)
  nn_box     the same with u in [-1, 1]
  nn_wide    NNDynamics(20, 4, [32]), T = 64, B = 1024, unbounded (the two-tile kernels)

The two routes alternate in one process after a warm-up solve of each; a solve is timed on the host clock from the call to a
device synchronise behind it (MPC.forward reads its convergence flags back, so host time is part of a solve).  The record
holds every repeat, the median and the spread (min, max).
usage: python tools/slew_bench.py [--rows lin,lin_box,pendulum,cartpole,nn,nn_box,nn_wide] [--rounds 7] [--rounds-off 3]"""
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


def lin_row(box, dev):
    from mpc import mpc
    from mpc.mpc import LinDx, QuadCost
    ns, nc, T, B, n = 12, 4, 50, 4096, 16
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    L = r(T, B, n, n)
    C = (L @ L.transpose(2, 3) / n + torch.eye(n)).to(dev)
    c = r(T, B, n).to(dev)
    F = (0.1 * r(T - 1, B, ns, n) + torch.cat((torch.eye(ns), torch.zeros(ns, nc)), 1)).to(dev)
    f = (0.1 * r(T - 1, B, ns)).to(dev)
    x0 = r(B, ns).to(dev)
    kw = dict(u_lower=-1.0, u_upper=1.0) if box else {}

    def make():
        return mpc.MPC(ns, nc, T, lqr_iter=5, verbose=-1, exit_unconverged=False, detach_unconverged=False, backprop=False,
                       slew_rate_penalty=1.0, eps=0.0, **kw)
    return make, (x0, QuadCost(C, c), LinDx(F, f)), dict(n_state=ns, n_ctrl=nc, T=T, B=B, lqr_iter=5, dtype="float32", box=box)


def sim_row(kind, dev):
    from mpc import mpc
    from mpc.env_dx import cartpole, pendulum
    from mpc.mpc import QuadCost
    dx = pendulum.PendulumDx() if kind == "pendulum" else cartpole.CartpoleDx()
    T, B = (20, 1024) if kind == "pendulum" else (25, 4096)
    ns = dx.n_state
    g = torch.Generator().manual_seed(2)
    th = (torch.rand(B, generator=g) - 0.5) * (3.0 if kind == "pendulum" else 0.6)
    zero = torch.zeros(B)
    x0 = (torch.stack((th.cos(), th.sin(), zero), 1) if kind == "pendulum" else torch.stack((zero, zero, th.cos(), th.sin(), zero), 1)).to(dev)
    q, p = dx.get_true_obj()
    cost = QuadCost(torch.diag(q).to(dev), p.to(dev))

    def make():
        return mpc.MPC(ns, 1, T, u_lower=dx.lower, u_upper=dx.upper, lqr_iter=10, verbose=-1, exit_unconverged=False,
                       detach_unconverged=False, backprop=False, n_batch=B, linesearch_decay=dx.linesearch_decay,
                       max_linesearch_iter=dx.max_linesearch_iter, grad_method=mpc.GradMethods.AUTO_DIFF, eps=0.0, slew_rate_penalty=0.5)
    return make, (x0, cost, dx), dict(kind=kind, T=T, B=B, lqr_iter=10, dtype="float32")


def nn_row(row, dev):
    from mpc import mpc
    from mpc.dynamics import NNDynamics
    from mpc.mpc import QuadCost
    ns, nc, hidden, T, B = (20, 4, [32], 64, 1024) if row == "nn_wide" else (12, 4, [100], 50, 4096)
    n = ns + nc
    torch.manual_seed(3)
    dyn = NNDynamics(ns, nc, hidden, activation="sigmoid").to(dev)
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    L = r(T, B, n, n)
    C = (L @ L.transpose(2, 3) / n + torch.eye(n)).to(dev)
    c = r(T, B, n).to(dev)
    x0 = r(B, ns).to(dev)
    kw = dict(u_lower=-1.0, u_upper=1.0) if row == "nn_box" else {}

    def make(flag=True):
        return mpc.MPC(ns, nc, T, lqr_iter=5, verbose=-1, exit_unconverged=False, detach_unconverged=False, backprop=False,
                       slew_rate_penalty=1.0, eps=0.0, grad_method=mpc.GradMethods.ANALYTIC, planned_network_slew=flag, **kw)
    return make, (x0, QuadCost(C, c), dyn), dict(n_state=ns, n_ctrl=nc, hidden=hidden, T=T, B=B, lqr_iter=5, dtype="float32",
                                                   box=row == "nn_box")


def solve_ms(ctrl, args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        out = ctrl(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="lin,lin_box,pendulum,cartpole")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rounds-off", type=int, default=3, help="repeats of the route-off solve of the simulator rows (seconds each)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "rows": {}}
    for row in a.rows.split(","):
        if row.startswith("nn"):
            make, args, meta = nn_row(row, dev)
            on, off = make(True), make(False)          # (the route is opt-in: off is the constructor's default)
        else:
            make, args, meta = (lin_row(row == "lin_box", dev) if row.startswith("lin") else sim_row(row, dev))
            on, off = make(), make()
            off._slew_plan = lambda *x, **k: None
        assert off.solve_route(*args).loop == "general"
        assert on.solve_route(*args).loop == "slew", "the predicate must fire on the new route"
        _, o_on = solve_ms(on, args)           # warm-up of either route at this shape
        _, o_off = solve_ms(off, args)
        rounds_off = a.rounds if row.startswith(("lin", "nn")) else a.rounds_off
        w_on, w_off = [], []
        for i in range(a.rounds):              # the routes alternate
            w_on.append(solve_ms(on, args)[0])
            if i < rounds_off:
                w_off.append(solve_ms(off, args)[0])
        rec = dict(meta)
        for name, w in (("route_on_ms", w_on), ("route_off_ms", w_off)):
            rec[name] = {"median": statistics.median(w), "min": min(w), "max": max(w), "repeats": w}
        rec["off_over_on"] = rec["route_off_ms"]["median"] / rec["route_on_ms"]["median"]
        rec["max_abs_du_between_routes"] = float((o_on[1] - o_off[1]).abs().max())
        rec["mean_cost_on"], rec["mean_cost_off"] = float(o_on[2].mean()), float(o_off[2].mean())
        res["rows"][row] = rec
        print(json.dumps({row: {k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median", "min", "max")}) for k, v in rec.items()}}), flush=True)
    out_dir = os.environ.get("MPC_BENCH_RECORD_DIR") or os.path.join(ROOT, "bench_records")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "slew_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
