#!/usr/bin/env python3
"""Timings of the row-per-problem kernel's CARRY instantiation (impl 10: a 16-lane row per problem for a simulator behind
MPC_ENV_CTRL_CARRY) against the lane-per-problem kernel (impl 4, what auto gives every carry call) on the GPU box, in one process.

Rows:
  step_pendulum_B   one pre-bound step around PendulumDx behind the carry (4 / 1), T = 20, B in {256, 1024, 4096, 8192}, the module's
                    bounds and line search, the simulator linearised inside the kernel: impl 10 against impl 4
  step_cartpole_B   the same around CartpoleDx (6 / 1), T = 25, B in {256, 1024, 2048, 4096}
  solve_pendulum    tools/slew_bench.py's `pendulum` row (B = 1024, T = 20, 10 iterations, gamma = 0.5, no-grad MPC.forward) with
                    `row_carry_kernel` on against off
  solve_cartpole_B  its `cartpole` row (T = 25) at B = 4096 and B = 2048, likewise

The two sides alternate after a warm-up of each.  A step repeat is `--inner` launches of the plan, a solve repeat `--inner-solve`
solves, timed on the host clock from the first call to a device synchronise behind the last and divided by their number (long
enough a window that the clocks have settled: the sustained state).  The record holds every repeat, the median and the spread
(min, max), what mpc_lqr_row_carry_pays says at that size, and `beats`: the slowest repeat of the row side below the fastest of
the lane side.
usage: python tools/row_carry_bench.py [--rows step_pendulum_1024,...] [--rounds 7] [--inner 1000] [--inner-solve 50]"""
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

STEP_B = {"pendulum": (256, 1024, 4096, 8192), "cartpole": (256, 1024, 2048, 4096)}
ALL_ROWS = (["step_%s_%d" % (k, B) for k in ("pendulum", "cartpole") for B in STEP_B[k]]
            + ["solve_pendulum_1024", "solve_cartpole_4096", "solve_cartpole_2048"])
GAMMA = 0.5


def sim_problem(kind, B, dev):
    """tools/slew_bench.py's simulator rows at batch B: the module, its start states, its own objective"""
    from mpc.env_dx import cartpole, pendulum
    dx = pendulum.PendulumDx() if kind == "pendulum" else cartpole.CartpoleDx()
    T = 20 if kind == "pendulum" else 25
    g = torch.Generator().manual_seed(2)
    th = (torch.rand(B, generator=g) - 0.5) * (3.0 if kind == "pendulum" else 0.6)
    zero = torch.zeros(B)
    x0 = (torch.stack((th.cos(), th.sin(), zero), 1) if kind == "pendulum" else torch.stack((zero, zero, th.cos(), th.sin(), zero), 1)).to(dev)
    q, p = dx.get_true_obj()
    return dx, T, x0, q.to(dev), p.to(dev)


def step_sides(row, dev):
    from mpc import _native
    from mpc._native import StepOptions
    _, kind, B = row.split("_")
    B = int(B)
    dx, T, x0, q, p = sim_problem(kind, B, dev)
    ns = dx.n_state
    be = _native.backend()
    env = dx.native_env().augmented()
    env.linearize = True
    Q = torch.diag(q).expand(T, B, ns + 1, ns + 1).contiguous()
    pp = p.expand(T, B, ns + 1).contiguous()
    aC, ac, _, _ = be.slew_augment(Q, pp, None, None, ns, 1, GAMMA)
    g = torch.Generator().manual_seed(5)
    u = (0.5 * float(dx.upper) * (2 * torch.rand(T, B, 1, generator=g) - 1)).to(dev)
    z0 = torch.cat((torch.zeros(B, 1, device=dev), x0), 1).contiguous()
    zs, _ = be.env_traj_cost(z0, u, env)
    opts = StepOptions(u_lower=float(dx.lower), u_upper=float(dx.upper), linesearch_decay=dx.linesearch_decay,
                       max_linesearch_iter=dx.max_linesearch_iter, true_dynamics=env)
    plans = {impl: be.plan_step(z0, aC, ac, None, None, zs.contiguous(), u, opts, impl=impl)
             for impl in (_native.IMPL_TINY, _native.IMPL_WAVE1_CARRY)}
    for impl, plan in plans.items():
        assert be.step_route(plan)[0] == impl
    # (impl 0 is impl 4 for every carry call)
    assert be.step_route(be.plan_step(z0, aC, ac, None, None, zs.contiguous(), u, opts))[0] == _native.IMPL_TINY

    def run(plan, inner):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            plan()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / inner
    r4, r10 = plans[_native.IMPL_TINY](), plans[_native.IMPL_WAVE1_CARRY]()
    torch.cuda.synchronize()
    meta = dict(kind=kind, T=T, B=B, dtype="float32", max_linesearch_iter=dx.max_linesearch_iter,
                row_carry_pays=bool(be.row_carry_pays(ns + 1, 1, torch.float32, T, B, opts, like=z0)),
                max_abs_du_between_sides=float((r4["new_u"] - r10["new_u"]).abs().max()),
                step_sizes_equal=float((r4["alphas"] == r10["alphas"]).float().mean()))
    return (lambda inner: run(plans[_native.IMPL_TINY], inner)), (lambda inner: run(plans[_native.IMPL_WAVE1_CARRY], inner)), meta, plans


def solve_sides(row, dev):
    from mpc import _native, mpc
    from mpc.mpc import QuadCost
    _, kind, B = row.split("_")
    B = int(B)
    dx, T, x0, q, p = sim_problem(kind, B, dev)
    args = (x0, QuadCost(torch.diag(q), p), dx)
    impls = []
    orig = _native.HipBackend.plan_step

    def spy(self, *a, **k):
        impls.append(k.get("impl", 0))
        return orig(self, *a, **k)

    def make(flag):
        return mpc.MPC(dx.n_state, 1, T, u_lower=dx.lower, u_upper=dx.upper, lqr_iter=10, verbose=-1, exit_unconverged=False,
                       detach_unconverged=False, backprop=False, n_batch=B, linesearch_decay=dx.linesearch_decay,
                       max_linesearch_iter=dx.max_linesearch_iter, grad_method=mpc.GradMethods.AUTO_DIFF, eps=0.0, slew_rate_penalty=GAMMA,
                       row_carry_kernel=flag)
    off, on = make(False), make(True)
    last = {}
    # which kernel the flag binds at this size (asked once, outside the timed windows)
    _native.HipBackend.plan_step = spy
    try:
        with torch.no_grad():
            on(*args)
    finally:
        _native.HipBackend.plan_step = orig
    bound = sorted(set(impls))

    def run(ctrl, name, inner):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(inner):
                last[name] = ctrl(*args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / inner
    meta = dict(kind=kind, T=T, B=B, lqr_iter=10, dtype="float32", gamma=GAMMA, flag_on_binds_impl=bound)
    return (lambda inner: run(off, "off", inner)), (lambda inner: run(on, "on", inner)), meta, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(ALL_ROWS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=1000)
    ap.add_argument("--inner-solve", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "rows": {}}
    for row in a.rows.split(","):
        solve = row.startswith("solve")
        lane, rowk, meta, keep = (solve_sides if solve else step_sides)(row, dev)
        inner = a.inner_solve if solve else a.inner
        lane(max(inner // 4, 2)), rowk(max(inner // 4, 2))          # warm-up of each side
        w_lane, w_row = [], []
        for _ in range(a.rounds):              # the sides alternate
            w_lane.append(lane(inner))
            w_row.append(rowk(inner))
        rec = dict(meta)
        names = ("flag_off_ms", "flag_on_ms") if solve else ("impl4_ms", "impl10_ms")
        for name, w in zip(names, (w_lane, w_row)):
            rec[name] = {"median": statistics.median(w), "min": min(w), "max": max(w), "repeats": w}
        rec["lane_over_row"] = rec[names[0]]["median"] / rec[names[1]]["median"]
        rec["beats"] = max(w_row) < min(w_lane)
        if solve:
            rec["max_abs_du_between_sides"] = float((keep["on"][1] - keep["off"][1]).abs().max())
            rec["max_rel_cost_between_sides"] = float((keep["on"][2] / keep["off"][2] - 1).abs().max())
        res["rows"][row] = rec
        print(json.dumps({row: {k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median", "min", "max")}) for k, v in rec.items()}}), flush=True)
        del lane, rowk, keep
        torch.cuda.empty_cache()
    out_dir = os.environ.get("MPC_BENCH_RECORD_DIR") or os.path.join(ROOT, "bench_records")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "row_carry_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
