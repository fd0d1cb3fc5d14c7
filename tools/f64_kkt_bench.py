#!/usr/bin/env python3
"""Timings of the float64 KKT backward with the closed-form part on the float64 wavefront kernels (MPC_KKT_GRADS_WAVE64,
csrc/kkt_wave64.hip) against the generic kernel that mpc_lqr_kkt_grads gives every float64 call, on the GPU box, in one process.

Rows (float64):
  f64_12_4        12/4, T = 50, B = 1024, unbounded (the README's float64 row)
  f64_12_4_box    the same, u* from a step under [-1, 1] (controls on a bound are pinned in the nested solve)
  f64_13_4        13/4, T = 50, B = 1024: odd n_state, the general form (4 bytes a lane)
  f64_32_8        32/8, T = 64, B = 1024: the two-slot ring

For each row two pairs, the sides of a pair alternating after one warm-up of each:
  backward    the whole HipBackend.kkt_backward (prepare, nested solve, closed-form part), grads_kernel off / on
  grads       the closed-form call alone on the same dx, du: mpc_lqr_kkt_grads / mpc_lqr_kkt_grads_kernel
A repeat is `--inner` calls timed on the host clock from the first call to a device synchronise behind the last, divided by their
number.  One line per row: median (min - max) of `--rounds` repeats, in milliseconds.
usage: python tools/f64_kkt_bench.py [--rows f64_12_4,...] [--rounds 7] [--inner 20]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc.pytorch_amd"))
sys.path.insert(0, ROOT)

ROWS = {"f64_12_4": (12, 4, 50, 1024, False), "f64_12_4_box": (12, 4, 50, 1024, True), "f64_13_4": (13, 4, 50, 1024, False),
        "f64_32_8": (32, 8, 64, 1024, False)}


def timed(call, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def alternate(sides, rounds, inner):
    """sides: {name: call} -> {name: the `rounds` repeats}, one warm-up of each first, the sides taking turns."""
    for call in sides.values():
        timed(call, 2)
    out = {name: [] for name in sides}
    for _ in range(rounds):
        for name, call in sides.items():
            out[name].append(timed(call, inner))
    return out


def summary(w):
    return "%.4f (%.4f - %.4f)" % (statistics.median(w), min(w), max(w))


def row_sides(row, dev):
    import bench
    from mpc import _native
    from mpc._native import KKT_GRADS_WAVE64, StepOptions
    ns, nc, T, B, box = ROWS[row]
    p = bench.make_problem(ns, nc, T, B, torch.float64, dev, seed=7 + ns, u_scale=0.3 if box else 0.0, clamp=1.0 if box else None)
    opts = StepOptions(**(dict(u_lower=-1.0, u_upper=1.0) if box else {}))
    be = _native.backend()
    L = _native.load()
    r = be.lqr_step(p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"], opts)
    g = torch.Generator(device=dev).manual_seed(6)
    gx = torch.randn(tuple(r["new_x"].shape), generator=g, device=dev, dtype=torch.float64)
    gu = torch.randn(tuple(r["new_u"].shape), generator=g, device=dev, dtype=torch.float64)
    args = (p["C"], p["c"], p["F"], p["f"], r["new_x"], r["new_u"], gx, gu, opts)
    backward = {"generic": lambda: be.kkt_backward(*args), "wave64": lambda: be.kkt_backward(*args, grads_kernel=KKT_GRADS_WAVE64)}
    # the closed-form call alone, on the nested solve's dx, du, into buffers of its own
    ref = be.kkt_backward(*args)
    prob, keep = be._problem(torch.zeros(B, ns, dtype=torch.float64, device=dev), p["C"], p["c"], p["F"], p["f"], r["new_x"], r["new_u"])
    outs = {side: {k: torch.empty_like(ref[k]) for k in ("dC", "dc", "dF", "df", "dx_init")} for side in ("generic", "wave64")}
    stream = torch.cuda.current_stream().cuda_stream

    def tail(o):
        return (ref["dx"].data_ptr(), ref["du"].data_ptr(), gx.data_ptr(), gu.data_ptr(), o["dC"].data_ptr(), o["dc"].data_ptr(),
                o["dF"].data_ptr(), o["df"].data_ptr(), o["dx_init"].data_ptr(), stream)
    assert int(L.mpc_lqr_kkt_grads_kernel_route(ctypes.byref(prob), KKT_GRADS_WAVE64, *tail(outs["wave64"])[:-1])) == KKT_GRADS_WAVE64

    def generic():
        assert L.mpc_lqr_kkt_grads(ctypes.byref(prob), *tail(outs["generic"])) == 0

    def wave64():
        assert L.mpc_lqr_kkt_grads_kernel(ctypes.byref(prob), KKT_GRADS_WAVE64, *tail(outs["wave64"])) == 0

    def differ():
        generic(), wave64()
        torch.cuda.synchronize()
        return max(float((outs["generic"][k] - outs["wave64"][k]).abs().max() / outs["generic"][k].abs().max().clamp(min=1.0))
                   for k in outs["generic"])
    meta = dict(n_state=ns, n_ctrl=nc, T=T, B=B, dtype="float64", box=box)
    if box:
        meta["share_on_a_bound"] = float((r["new_u"].abs() == 1.0).double().mean())
    return backward, {"generic": generic, "wave64": wave64}, meta, differ, (keep, ref)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "rows": {}}
    for row in a.rows.split(","):
        backward, grads, meta, differ, keep = row_sides(row, dev)
        rec = dict(meta)
        for pair, sides in (("backward", backward), ("grads", grads)):
            rec[pair] = alternate(sides, a.rounds, a.inner)
        rec["max_difference_over_largest_entry"] = differ()
        res["rows"][row] = rec
        med = lambda pair, side: statistics.median(rec[pair][side])
        print("%s: backward generic %s wave64 %s ms [x%.2f] | grads generic %s wave64 %s ms [x%.2f] | "
              "max difference %.2e of the largest entry%s"
              % (row, summary(rec["backward"]["generic"]), summary(rec["backward"]["wave64"]), med("backward", "generic") / med("backward", "wave64"),
                 summary(rec["grads"]["generic"]), summary(rec["grads"]["wave64"]), med("grads", "generic") / med("grads", "wave64"),
                 rec["max_difference_over_largest_entry"],
                 " | %.0f %% of the controls on a bound" % (100 * meta["share_on_a_bound"]) if meta["box"] else ""), flush=True)
        del backward, grads, differ, keep
        torch.cuda.empty_cache()
    out_dir = os.environ.get("MPC_BENCH_RECORD_DIR") or os.path.join(ROOT, "bench_records")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "f64_kkt_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
