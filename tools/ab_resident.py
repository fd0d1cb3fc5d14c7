#!/usr/bin/env python3
"""Paired timing of the headline 12/4 step (float32, T = 50, vouched, two alternating problem sets as bench.py times it) on the
two-slot-ring build and on the resident-F build (csrc/lqr_dpp16_res.o), in ONE process: MPC_DPP16_RESIDENT is flipped between
repetitions (the library re-reads it at every launch under MPC_DPP16_RING_DYNAMIC), the two sides take turns, each repetition is
`--launches` launches bracketed by one pair of HIP events.  Positions within a job differ by up to 2 us (docs/history/r18.md), so
only paired runs count, and the gain counts only if the SLOWEST resident repetition is faster than the FASTEST parent one.

  python tools/ab_resident.py [--batch 4096 2048] [--reps 7] [--launches 200] [--settle 200] [--json out.json]

Prints one JSON line per batch."""
import argparse
import json
import os
import sys

os.environ.setdefault("MPC_DPP16_RING_DYNAMIC", "1")          # before the library loads: the switch follows the environment
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mpc.pytorch_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[4096, 2048])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--settle", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from mpc import _native
    from mpc._native import StepOptions
    be = _native.HipBackend()
    L = _native.load()
    dev = "cuda:0"
    rows = []
    for B in args.batch:
        psets = [bench.make_problem(12, 4, args.horizon, B, torch.float32, dev, seed=7919 * i, u_scale=0.0, clamp=None) for i in range(2)]
        opts = StepOptions(nominal_on_dynamics=True, c_symmetric=True)
        plans = [be.plan_step(q["x_init"], q["C"], q["c"], q["F"], q["f"], q["cur_x"], q["cur_u"], opts) for q in psets]
        turn = 0

        def run(n, resident):
            nonlocal turn
            os.environ["MPC_DPP16_RESIDENT"] = "1" if resident else "0"
            n0 = L.mpc_lqr_resident_launches()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                plans[turn]()
                turn ^= 1
            b.record()
            torch.cuda.synchronize()
            assert L.mpc_lqr_resident_launches() - n0 == (n if resident else 0), "the switch did not reach the launcher"
            return a.elapsed_time(b) * 1e3 / n          # us per launch

        for side in (0, 1):
            run(args.settle // 2, side)
        us = {0: [], 1: []}
        for rep in range(args.reps):
            for side in ((0, 1) if rep % 2 == 0 else (1, 0)):          # (who goes first alternates too)
                us[side].append(run(args.launches, side))
        # the two builds must agree bit for bit on the last set they both ran
        outs = []
        for side in (0, 1):
            os.environ["MPC_DPP16_RESIDENT"] = str(side)
            r = plans[0]()
            torch.cuda.synchronize()
            outs.append({k: r[k].clone() for k in ("new_x", "new_u", "costs", "alphas")})
        same = all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])
        med = lambda v: sorted(v)[len(v) // 2]
        row = {"B": B, "T": args.horizon, "launches_per_rep": args.launches, "settle": args.settle,
               "parent_us": [round(x, 2) for x in us[0]], "resident_us": [round(x, 2) for x in us[1]],
               "parent_median_us": round(med(us[0]), 2), "resident_median_us": round(med(us[1]), 2),
               "gain_us": round(med(us[0]) - med(us[1]), 2),
               "slowest_resident_below_fastest_parent": max(us[1]) < min(us[0]), "bit_identical": same}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
