#!/usr/bin/env python3
"""Timings of the float64 weight gradient of the NNDynamics linearisation on the GPU box: `mpc.MPC(f64_weight_grad_kernel=True)`
(mpc_mlp_linearize_dtype forward, mpc_mlp_param_grad_dtype backward -- csrc/nn_param_grad64.h) against the module + autograd
route in the same process, which is the same controller with the flag off.

Rows (sigmoid, hidden [100], B = 1024):
  nn12   NNDynamics(12, 4, [100]), T = 50
  nn32   NNDynamics(32, 8, [100]), T = 64

Per row, each with device events, the two routes alternating, median (min - max) of `--rounds` windows after a run-up of each:
  linearize_fwd_bwd   MPC.linearize_dynamics(diff=True) at (T-1) B random points + backward of fixed cotangents
  c_call              HipBackend.mlp_linearize_backward64 alone (the C call and its output / workspace allocations)
  solve_fwd_bwd       forward + backward of a 5-iteration solve (eps = 0, loss on u)
A window of the kernel route is `--reps` calls, a window of the module route one.
usage: python tools/nn_f64_grad_bench.py [--rows nn12,nn32] [--rounds 7] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc.pytorch_amd"))
sys.path.insert(0, ROOT)

SHAPES = {"nn12": (12, 4, 50, 1024), "nn32": (32, 8, 64, 1024)}
F64 = torch.float64


def timed(fn, reps):
    """device milliseconds per call of `reps` back-to-back calls"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(w):
    return {"median": statistics.median(w), "min": min(w), "max": max(w), "repeats": w}


def alternate(on, off, rounds, reps):
    on(); off()                                            # run-up of either route
    w_on, w_off = [], []
    for _ in range(rounds):
        w_on.append(timed(on, reps))
        w_off.append(timed(off, 1))
    return summary(w_on), summary(w_off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="nn12,nn32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    from mpc import _native, mpc
    from mpc.dynamics import NNDynamics
    from mpc.mpc import GradMethods, QuadCost
    dev = "cuda:0"
    be = _native.backend()
    res = {"device": torch.cuda.get_device_name(0), "rows": {}}
    for row in a.rows.split(","):
        ns, nc, T, B = SHAPES[row]
        n = ns + nc
        torch.manual_seed(3)
        dx = NNDynamics(ns, nc, [100], activation="sigmoid").double().to(dev)
        params = list(dx.fcs.parameters())
        g = torch.Generator().manual_seed(4)
        r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
        Lc = r(T, B, n, n)
        C = (Lc @ Lc.transpose(2, 3) / n + torch.eye(n, dtype=F64)).to(dev)
        c, x0 = r(T, B, n).to(dev), r(B, ns).to(dev)
        xs, us = r(T, B, ns).to(dev), r(T, B, nc).to(dev)
        gF, gf = r(T - 1, B, ns, n).to(dev), r(T - 1, B, ns).to(dev)
        kw = dict(lqr_iter=5, verbose=-1, exit_unconverged=False, detach_unconverged=False, eps=0.0, grad_method=GradMethods.ANALYTIC)
        ctrl = {flag: mpc.MPC(ns, nc, T, f64_weight_grad_kernel=flag, **kw) for flag in (True, False)}
        assert ctrl[True]._param_grad_net(dx, xs) is not None and ctrl[False]._param_grad_net(dx, xs) is None
        weights = torch.linspace(-1, 1, nc, device=dev, dtype=F64)

        def linearize(flag):
            def run():
                F, f = ctrl[flag].linearize_dynamics(xs, us, dx, diff=True)
                return torch.autograd.grad((F * gF).sum() + (f * gf).sum(), params)
            return run

        def solve(flag):
            def run():
                x, u, _ = ctrl[flag](x0, QuadCost(C, c), dx)
                return torch.autograd.grad((u ** 2).sum() + (u * weights).sum(), params)
            return run
        rec = dict(n_state=ns, n_ctrl=nc, hidden=[100], T=T, B=B, points=(T - 1) * B, dtype="float64")
        g_on, g_off = linearize(True)(), linearize(False)()
        rec["linearize_max_rel_diff"] = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(g_on, g_off))
        rec["linearize_fwd_bwd_kernel_ms"], rec["linearize_fwd_bwd_module_ms"] = alternate(linearize(True), linearize(False), a.rounds, a.reps)
        net = dx.native_net(xs)
        px, pu = xs[:-1].reshape(-1, ns).contiguous(), us[:-1].reshape(-1, nc).contiguous()
        pF, pf = gF.reshape(-1, ns, n), gf.reshape(-1, ns)
        call = lambda: be.mlp_linearize_backward64(net, px, pu, pF, pf)
        call()
        rec["c_call_ms"] = summary([timed(call, a.reps) for _ in range(a.rounds)])
        fwd = lambda: be.mlp_linearize(net, px, pu)
        fwd()
        rec["forward_call_ms"] = summary([timed(fwd, a.reps) for _ in range(a.rounds)])
        s_on, s_off = solve(True)(), solve(False)()
        rec["solve_max_rel_diff"] = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(s_on, s_off))
        rec["solve_fwd_bwd_kernel_ms"], rec["solve_fwd_bwd_module_ms"] = alternate(solve(True), solve(False), a.rounds, 1)
        res["rows"][row] = rec
        print(json.dumps({row: {k: (v if not (isinstance(v, dict) and "repeats" in v) else {q: round(v[q], 3) for q in ("median", "min", "max")})
                                for k, v in rec.items()}}), flush=True)
    out_dir = os.environ.get("MPC_BENCH_RECORD_DIR") or os.path.join(ROOT, "bench_records")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "nn_f64_grad_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
