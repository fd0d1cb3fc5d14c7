#!/usr/bin/env python3
"""Timings of the fused KKT backward on ONE state tile (MPC_KKT_MFMA40_NARROW16 / _NARROW4, asked for as the family
KKT_PREFER_NARROW) against the padded two-tile kernel that kernel = 0 picks for the same call, on the GPU box, in one process.

Rows:
  kkt_16_4 / kkt_16_4_box       one pre-bound backward (plan_kkt_backward, C vouched symmetric), 16/4, B = 4096, T = 50, unbounded /
                                u* from a step under [-1, 1] (controls on a bound are pinned)
  kkt_13_4                      the same at 13/4, B = 1024 (dword gathers), unbounded
  kkt_16_8                      the same at 16/8, B = 1024, unbounded
  solve                         one MPC.forward + backward of a 12/4, B = 4096, T = 50, 5-iteration, gamma = 1 slew-rate solve (the
                                augmentation makes it 16/4) with `narrow_kkt_kernel` off and on.  Off, the slew ending makes no symmetry
                                promise and its backward is the three-call route; on, it is the one-tile fused kernel.

Both kernels of a backward row are followed by the same memory-bound kkt_outer_kernel, which is part of the call and of the time.
The two sides alternate after one warm-up of each.  A backward repeat is `--inner` calls of the plan, timed on the host clock from
the first call to a device synchronise behind the last, divided by their number; a solve repeat is one forward + backward to a
device synchronise.  The record holds every repeat, the median and the spread (min, max); `beats` says whether the slowest repeat
of the narrow side lies below the fastest of the wide side.
usage: python tools/narrow_kkt_bench.py [--rows kkt_16_4,...] [--rounds 7] [--inner 20]"""
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

KKT_ROWS = {"kkt_16_4": (16, 4, 4096, False), "kkt_16_4_box": (16, 4, 4096, True), "kkt_13_4": (13, 4, 1024, False),
            "kkt_16_8": (16, 8, 1024, False)}
ALL_ROWS = list(KKT_ROWS) + ["solve"]


def kkt_sides(row, dev):
    import bench
    from mpc import _native
    from mpc._native import StepOptions
    ns, nc, B, box = KKT_ROWS[row]
    T = 50
    p = bench.make_problem(ns, nc, T, B, torch.float32, dev, seed=7 + ns, u_scale=0.3 if box else 0.0, clamp=1.0 if box else None)
    opts = StepOptions(c_symmetric=True, **(dict(u_lower=-1.0, u_upper=1.0) if box else {}))
    be = _native.backend()
    r = be.lqr_step(p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"], opts)
    g = torch.Generator(device=dev).manual_seed(6)
    gx = torch.randn(tuple(r["new_x"].shape), generator=g, device=dev)
    gu = torch.randn(tuple(r["new_u"].shape), generator=g, device=dev)
    args = (p["C"], p["c"], p["F"], p["f"], r["new_x"], r["new_u"], gx, gu, opts)
    wide = be.plan_kkt_backward(*args)
    narrow = be.plan_kkt_backward(*args, kernel=_native.KKT_PREFER_NARROW)
    sixteen = ns % 4 == 0 and nc % 4 == 0
    assert wide.kernel == (_native.KKT_MFMA40_PAD16 if sixteen else _native.KKT_MFMA40_PAD4), wide.kernel
    assert narrow.kernel == (_native.KKT_MFMA40_NARROW16 if sixteen else _native.KKT_MFMA40_NARROW4), narrow.kernel

    def run(plan, inner):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            plan()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / inner
    meta = dict(n_state=ns, n_ctrl=nc, T=T, B=B, dtype="float32", box=box, wide_kernel=wide.kernel, narrow_kernel=narrow.kernel)
    if box:
        meta["share_on_a_bound"] = float((r["new_u"].abs() == 1.0).float().mean())

    def differ():
        a, b = wide(), narrow()
        torch.cuda.synchronize()
        return max(float((a[k] - b[k]).abs().max()) for k in ("dx_init", "dC", "dc", "dF", "df"))
    return (lambda inner: run(wide, inner)), (lambda inner: run(narrow, inner)), meta, differ


def solve_sides(row, dev):
    from mpc import mpc
    from mpc.mpc import LinDx, QuadCost
    ns, nc, T, B, n = 12, 4, 50, 4096, 16
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    L = r(T, B, n, n)
    C = (L @ L.transpose(2, 3) / n + torch.eye(n)).to(dev).requires_grad_(True)
    c = r(T, B, n).to(dev).requires_grad_(True)
    F = (0.1 * r(T - 1, B, ns, n) + torch.cat((torch.eye(ns), torch.zeros(ns, nc)), 1)).to(dev).requires_grad_(True)
    f = (0.1 * r(T - 1, B, ns)).to(dev).requires_grad_(True)
    x0 = r(B, ns).to(dev)

    def make(flag):
        return mpc.MPC(ns, nc, T, lqr_iter=5, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                       slew_rate_penalty=1.0, eps=0.0, narrow_kkt_kernel=flag)
    off, on = make(False), make(True)
    last = {}

    def run(ctrl, name):
        for t in (C, c, F, f):
            t.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, u, _ = ctrl(x0, QuadCost(C, c), LinDx(F, f))
        (x.sum() + u.sum()).backward()
        torch.cuda.synchronize()
        last[name] = C.grad
        return (time.perf_counter() - t0) * 1e3
    meta = dict(n_state=ns, n_ctrl=nc, T=T, B=B, lqr_iter=5, dtype="float32", box=False, gamma=1.0)
    return (lambda inner: run(off, "off")), (lambda inner: run(on, "on")), meta, lambda: float((last["on"] - last["off"]).abs().max())


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
        wide, narrow, meta, differ = (solve_sides if row == "solve" else kkt_sides)(row, dev)
        wide(2), narrow(2)                     # one warm-up of each side
        ww, wn = [], []
        for _ in range(a.rounds):              # the sides alternate
            ww.append(wide(a.inner))
            wn.append(narrow(a.inner))
        rec = dict(meta)
        names = ("flag_off_ms", "flag_on_ms") if row == "solve" else ("wide_ms", "narrow_ms")
        for name, w in zip(names, (ww, wn)):
            rec[name] = {"median": statistics.median(w), "min": min(w), "max": max(w), "repeats": w}
        rec["wide_over_narrow"] = rec[names[0]]["median"] / rec[names[1]]["median"]
        rec["beats"] = max(wn) < min(ww)
        rec["max_abs_difference_between_sides"] = differ()
        res["rows"][row] = rec
        print(json.dumps({row: {k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median", "min", "max")}) for k, v in rec.items()}}), flush=True)
        del wide, narrow, differ
        torch.cuda.empty_cache()
    out_dir = os.environ.get("MPC_BENCH_RECORD_DIR") or os.path.join(ROOT, "bench_records")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "narrow_kkt_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
