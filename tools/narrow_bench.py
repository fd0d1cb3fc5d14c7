#!/usr/bin/env python3
"""Timings of the NARROW instantiation of the padded 32/8 kernel (impl 9: one 16-row state tile, n_state <= 16) against the padded
kernel itself (impl 7) on the GPU box, in one process.

Rows:
  step_16_4 / step_16_4_box     one pre-bound step (vouched nominal, symmetric C), 16/4, B = 4096, T = 50, unbounded / u in [-1, 1]
  step_13_4 / step_13_4_box     the same at 13/4, B = 1024 (dword gathers)
  step_16_8 / step_16_8_box     the same at 16/8, B = 1024
  solve / solve_box             the 12/4, B = 4096, T = 50, 5-iteration, gamma = 1 no-grad MPC.forward of tools/slew_bench.py's `lin`
                                rows (the augmentation makes it 16/4) with `narrow_step_kernel` off and on

The two sides alternate after one warm-up of each.  A step repeat is `--inner` launches of the plan, timed on the host clock from
the first call to a device synchronise behind the last, divided by their number; a solve repeat is one MPC.forward to a device
synchronise.  The record holds every repeat, the median and the spread (min, max); `beats` says whether the slowest repeat of
the narrow side lies below the fastest of the padded side.
usage: python tools/narrow_bench.py [--rows step_16_4,...] [--rounds 7] [--inner 20]"""
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

STEP_ROWS = {"step_16_4": (16, 4, 4096), "step_13_4": (13, 4, 1024), "step_16_8": (16, 8, 1024)}
ALL_ROWS = [r + s for r in STEP_ROWS for s in ("", "_box")] + ["solve", "solve_box"]


def step_sides(row, dev):
    import bench
    from mpc import _native
    from mpc._native import StepOptions
    box = row.endswith("_box")
    ns, nc, B = STEP_ROWS[row[:-4] if box else row]
    T = 50
    p = bench.make_problem(ns, nc, T, B, torch.float32, dev, seed=7 + ns, u_scale=0.3 if box else 0.0, clamp=1.0 if box else None)
    kw = dict(u_lower=-1.0, u_upper=1.0) if box else {}
    be = _native.backend()
    args = (p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"])
    opts = StepOptions(nominal_on_dynamics=True, c_symmetric=True, **kw)
    plans = {impl: be.plan_step(*args, opts, impl=impl) for impl in (_native.IMPL_MFMA40_PAD, _native.IMPL_MFMA40_NARROW)}
    for impl, plan in plans.items():
        assert be.step_route(plan)[0] == impl
    p7, p9 = plans[_native.IMPL_MFMA40_PAD], plans[_native.IMPL_MFMA40_NARROW]

    def run(plan, inner):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            plan()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / inner
    meta = dict(n_state=ns, n_ctrl=nc, T=T, B=B, dtype="float32", box=box)
    return (lambda inner: run(p7, inner)), (lambda inner: run(p9, inner)), meta, (p, plans)


def solve_sides(row, dev):
    from mpc import mpc
    from mpc.mpc import LinDx, QuadCost
    box = row.endswith("_box")
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
    args = (x0, QuadCost(C, c), LinDx(F, f))

    def make(flag):
        return mpc.MPC(ns, nc, T, lqr_iter=5, verbose=-1, exit_unconverged=False, detach_unconverged=False, backprop=False,
                       slew_rate_penalty=1.0, eps=0.0, narrow_step_kernel=flag, **kw)
    off, on = make(False), make(True)
    last = {}

    def run(ctrl, name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            last[name] = ctrl(*args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    meta = dict(n_state=ns, n_ctrl=nc, T=T, B=B, lqr_iter=5, dtype="float32", box=box, gamma=1.0)
    return (lambda inner: run(off, "off")), (lambda inner: run(on, "on")), meta, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(ALL_ROWS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "rows": {}}
    for row in a.rows.split(","):
        wide, narrow, meta, keep = (solve_sides if row.startswith("solve") else step_sides)(row, dev)
        wide(2), narrow(2)                     # one warm-up of each side
        w7, w9 = [], []
        for _ in range(a.rounds):              # the sides alternate
            w7.append(wide(a.inner))
            w9.append(narrow(a.inner))
        rec = dict(meta)
        names = ("flag_off_ms", "flag_on_ms") if row.startswith("solve") else ("impl7_ms", "impl9_ms")
        for name, w in zip(names, (w7, w9)):
            rec[name] = {"median": statistics.median(w), "min": min(w), "max": max(w), "repeats": w}
        rec["wide_over_narrow"] = rec[names[0]]["median"] / rec[names[1]]["median"]
        rec["beats"] = max(w9) < min(w7)
        if row.startswith("solve"):
            rec["max_abs_du_between_sides"] = float((keep["on"][1] - keep["off"][1]).abs().max())
        res["rows"][row] = rec
        print(json.dumps({row: {k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median", "min", "max")}) for k, v in rec.items()}}), flush=True)
        del wide, narrow, keep
        torch.cuda.empty_cache()
    out_dir = os.environ.get("MPC_BENCH_RECORD_DIR") or os.path.join(ROOT, "bench_records")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "narrow_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
