#!/usr/bin/env python3
"""Timings of the backward of a solve whose cost and linear model are SHARED by the batch (C [T,n,n], c [T,n], F [T-1,ns,n],
f [T-1,ns], all four learnable, a scalar loss on x and u) on the GPU box: `shared_grad_kernel=True` (lqr_step._LQRStepSharedFn,
mpc_lqr_kkt_grads_shared: the gradients summed over the batch inside the kernels) against the flag off -- the route of the
commit before: stride-0 views, per-problem dC / dF blocks, autograd's sum through the expand.

Rows: 12/4, T = 50, B = 4096 and 32/8, T = 64, B = 1024, float32, each box-constrained (u in [-0.5, 0.5]) and unconstrained.

What is timed is the backward of the no-op step (`LQRStep(..., no_op_forward=True)` at the solution of a five-iteration solve,
`c_symmetric=True` as mpc.MPC vouches after its first iteration): torch.autograd.grad of the loss with respect to the four
leaves, `--calls` of them between two HIP events, so host time (allocations, struct building, the autograd engine) is part of
the figure as it is part of a user's.  The two routes alternate in one process after `--warmup` windows of each; the record
holds every window, the median and the spread (min, max) per call.  `entry_ms` is the new C entry alone (costates, GEMM over
the batch, the final sum: three launches, pre-bound arguments) the same way.  `bytes` counts what the two routes move through
HBM for the gradients, from the shapes.
usage: python tools/shared_grad_bench.py [--rows 12_4,12_4_box,32_8,32_8_box] [--rounds 7] [--calls 10] [--warmup 3]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc.pytorch_amd"))
sys.path.insert(0, ROOT)

SHAPES = {"12_4": (12, 4, 50, 4096), "32_8": (32, 8, 64, 1024)}


def problem(ns, nc, T, B, dev):
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    n = ns + nc
    L = r(T, n, n) / n ** 0.5
    C = L.transpose(1, 2) @ L + torch.eye(n)
    F = torch.cat((0.9 * torch.eye(ns).expand(T - 1, ns, ns) + 0.3 * r(T - 1, ns, ns) / ns ** 0.5, 0.5 * r(T - 1, ns, nc)), 2)
    base = dict(C=0.5 * (C + C.transpose(1, 2)), c=r(T, n), F=F, f=0.2 * r(T - 1, ns))
    return {k: v.to(dev) for k, v in base.items()}, r(B, ns).to(dev), r(T, B, ns).to(dev), r(T, B, nc).to(dev)


def window_ms(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="12_4,12_4_box,32_8,32_8_box")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    from mpc import _native, mpc
    from mpc.lqr_step import LQRStep, _expand_shared
    from mpc.mpc import LinDx, QuadCost
    dev = "cuda:0"
    be = _native.backend()
    L = _native.load()
    res = {"device": torch.cuda.get_device_name(0), "rows": {}}
    for row in a.rows.split(","):
        box = row.endswith("_box")
        ns, nc, T, B = SHAPES[row[:-4] if box else row]
        n = ns + nc
        base, x0, wx, wu = problem(ns, nc, T, B, dev)
        kw = dict(u_lower=-0.5, u_upper=0.5) if box else {}
        with torch.no_grad():
            x, u, _ = mpc.MPC(ns, nc, T, lqr_iter=5, verbose=-1, exit_unconverged=False, detach_unconverged=False, n_batch=B, **kw)(
                x0, QuadCost(base["C"], base["c"]), LinDx(base["F"], base["f"]))
        names = ("C", "c", "F", "f")

        def route(flag):
            leaves = [base[k].clone().requires_grad_(True) for k in names]
            args = leaves if flag else [_expand_shared(t, k, T, B) for k, t in enumerate(leaves)]      # flag off: the views MPC.forward makes
            step = LQRStep(ns, nc, T, current_x=x, current_u=u, no_op_forward=True, c_symmetric=True, shared_grad_kernel=flag, **kw)
            xo, uo = step(x0, *args)
            loss = (xo * wx).sum() + (uo * wu).sum()
            return lambda: torch.autograd.grad(loss, leaves, retain_graph=True)
        on, off = route(True), route(False)
        # the new entry alone, arguments bound once
        Cv, cv, Fv, fv = (_expand_shared(base[k], i, T, B) for i, k in enumerate(names))
        g = be.kkt_backward_shared(Cv, cv, Fv, fv, x, u, wx, wu, _native.StepOptions(c_symmetric=True, **kw))
        p, keep = be._problem(x[0], Cv, cv, Fv, fv, x, u)
        nbytes = int(L.mpc_lqr_kkt_shared_workspace_bytes(ctypes.byref(p)))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        outs = [torch.empty_like(g[k]) for k in ("sum_dC", "sum_dc", "sum_dF", "sum_df")]
        dxi = torch.empty(B, ns, device=dev)
        stream = _native._stream(x.device)
        eargs = (ctypes.byref(p), g["dx"].data_ptr(), g["du"].data_ptr(), wx.data_ptr(), wu.data_ptr(), *[o.data_ptr() for o in outs],
                 dxi.data_ptr(), ws.data_ptr(), nbytes, stream)

        def entry():
            rc = L.mpc_lqr_kkt_grads_shared(*eargs)
            assert rc == 0, L.mpc_lqr_last_error()
        for _ in range(a.warmup):              # the run-up of every route at this shape
            window_ms(on, a.calls); window_ms(off, a.calls); window_ms(entry, a.calls)
        w = {"flag_on_ms": [], "flag_off_ms": [], "entry_ms": []}
        for _ in range(a.rounds):              # the routes alternate
            t, g_on = window_ms(on, a.calls); w["flag_on_ms"].append(t)
            t, g_off = window_ms(off, a.calls); w["flag_off_ms"].append(t)
            w["entry_ms"].append(window_ms(entry, a.calls)[0])
        rec = dict(n_state=ns, n_ctrl=nc, T=T, B=B, box=box, dtype="float32", calls_per_window=a.calls)
        for name, v in w.items():
            rec[name] = {"median": statistics.median(v), "min": min(v), "max": max(v), "repeats": v}
        rec["off_over_on"] = rec["flag_off_ms"]["median"] / rec["flag_on_ms"]["median"]
        rec["max_rel_diff_between_routes"] = {k: float((p_ - q_).abs().max() / q_.abs().max()) for k, p_, q_ in zip(names, g_on, g_off)}
        per_problem = T * B * (n * n + n) * 4 + (T - 1) * B * (ns * n + ns) * 4
        rec["bytes"] = {"per_problem_gradients_written_then_read": per_problem,
                        "summed_route_inputs": T * B * 2 * n * 4 + (T - 1) * B * 2 * ns * 4, "summed_route_workspace": nbytes}
        res["rows"][row] = rec
        print(json.dumps({row: {k: (v if not (isinstance(v, dict) and "median" in v) else {q: round(v[q], 4) for q in ("median", "min", "max")})
                                for k, v in rec.items()}}), flush=True)
    out_dir = os.environ.get("MPC_BENCH_RECORD_DIR") or os.path.join(ROOT, "bench_records")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "shared_grad_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
