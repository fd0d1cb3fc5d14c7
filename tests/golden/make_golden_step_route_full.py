"""The WHOLE route of the step entry (csrc/capi.hip: step_route -- kernel, phase, ring, pad16, needs_resolve, every workspace offset,
the qp record, code and text of a refusal, and what mpc_lqr_step_route answers in front of it) over a grid of made-up calls, as
tests/step_route_probe.cpp prints it, WITHOUT a device.  step_route_answers.json pins refusals and (kernel, ring); this table pins
everything step_impl patches its launch from, simulators included.

The table (step_route_full.json) is recorded from a build of the commit BEFORE the step kernels were gathered into one table
(docs/history/r22.md): build that commit somewhere, then

    MPC_LQR_HIP_LIB=/path/to/that/libmpc_lqr_hip.so python tests/golden/make_golden_step_route_full.py

It holds one SHA-256 per cell (n_state, n_ctrl, dtype, impl) over the probe's lines of that cell's calls, in the order `calls` gives
them.  tests/test_step_route_host.py recomputes every digest on the library under test and compares exactly.  The probe reads eighteen
integers per call (its header names them); the library assumes 1024 SIMDs where no device answers, which is where the batch rules sit.

The grid, per cell:
  simulators   at [T,B] = [5,3]: (none, kind 1..3 each plain / carry / linearize / both -- whichever n_state the shape has, so matching and
               not) x sweep_only x gains (none, both, K alone) x workspace (none, full, 4 bytes off, the padded gains' bytes only).
               Thinned where it tells nothing: MPC_OPT_SWEEP_ONLY with a simulator is refused by one check of the call in front of every
               kernel's, so under sweep_only only "none" and the first and the last simulator variant stay (153,444 calls in all,
               about 0.6 s; the whole product would be 212,724)
  options      at [5,3]: bounds (none, scalar, tensor) x mask x max_linesearch_iter (10, 17) x align (16, 4) x the four workspaces,
               no gains, no status words (so they are parked)
  batches      the shapes a batch rule governs, under impl 0 and the kernel's own code, bounds none / scalar: 12/4 and 32/8 on either
               side of B = 1024, 1536 and 4096 (with and without a mask); the one-control shapes 3/1 .. 6/1 on either side of every
               multiple of 1024 up to 8192 at T = 5 and T = 200 (the row kernel's "pays" limit moves with its LDS), without a simulator
               and with each kind, plain and carry
  phases       impl 1 alone: the sweep and rollout entries (phase 1, 2), no workspace, gains none / both / K alone
"""
import hashlib
import importlib.util
import itertools
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "mpc.pytorch_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

_spec = importlib.util.spec_from_file_location("make_golden_step_route", os.path.join(HERE, "make_golden_step_route.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

OUT = os.path.join(HERE, "step_route_full.json")
SHAPES = gen.SHAPES + ((4, 1), (5, 1), (16, 4), (16, 8), (8, 6))
IMPLS = tuple(range(-1, 12))
SIMS = ((0, 0, 0),) + tuple((kind, carry, lin) for kind in (1, 2, 3) for carry in (0, 1) for lin in (0, 1))
NO_WS, FULL, OFF, GAINS_ONLY = 0, 1, 2, 3
ROW_SHAPES = ((3, 1), (4, 1), (5, 1), (6, 1))
OWN = {(12, 4): 3, (32, 8): 5}                      # the kernel whose ring a batch rule picks
RING_B = (1024, 1025, 1536, 1537, 4096, 4097)
ROW_B = tuple(b for m in range(1, 9) for b in (1024 * m, 1024 * m + 1))


def call(ns, nc, f64, impl, T=5, B=3, bounds=0, mask=0, max_ls=10, sweep=0, gains=0, ws=FULL, align=16, status=1, sim=(0, 0, 0), phase=3):
    return (ns, nc, f64, T, B, bounds, mask, max_ls, sweep, gains, ws, align, impl, status) + tuple(sim) + (phase,)


def products(ns, nc, f64, impl):
    """The two products every cell has."""
    c = [call(ns, nc, f64, impl, sim=sim, sweep=sweep, gains=gains, ws=ws)
         for sim, sweep, gains, ws in itertools.product(SIMS, (0, 1), (0, 1, 2), (NO_WS, FULL, OFF, GAINS_ONLY))
         if not sweep or sim in (SIMS[0], SIMS[1], SIMS[-1])]
    c += [call(ns, nc, f64, impl, bounds=bounds, mask=mask, max_ls=max_ls, align=align, ws=ws, status=0)
          for bounds, mask, max_ls, align, ws in itertools.product((0, 1, 2), (0, 1), (10, 17), (16, 4), (NO_WS, FULL, OFF, GAINS_ONLY))]
    return c


def rules(ns, nc, f64, impl):
    """... and the calls of the cells a batch rule or a phase governs."""
    c = []
    if (ns, nc) in OWN and impl in (0, OWN[(ns, nc)]):
        c += [call(ns, nc, f64, impl, B=B, bounds=bounds, mask=mask) for B, bounds, mask in itertools.product(RING_B, (0, 1), (0, 1))]
    if (ns, nc) in ROW_SHAPES and impl in (0, 6, 10):
        c += [call(ns, nc, f64, impl, T=T, B=B, bounds=bounds, sim=sim)
              for T, B, bounds, sim in itertools.product((5, 200), ROW_B, (0, 1), [s for s in SIMS if not s[2]])]
    if impl == 1:
        c += [call(ns, nc, f64, impl, ws=NO_WS, gains=gains, phase=phase) for phase, gains in itertools.product((1, 2), (0, 1, 2))]
    return c


def calls(ns, nc, f64, impl):
    """The calls of one cell, in the order their lines are hashed in."""
    return products(ns, nc, f64, impl) + rules(ns, nc, f64, impl)


def as_text(cs):
    return "".join(" ".join(map(str, c)) + "\n" for c in cs)


PRODUCTS = as_text(products("@n", "@c", "@d", "@i"))          # (their text once, the cell filled in)
N_PRODUCTS = PRODUCTS.count("\n")


def cell_text(ns, nc, f64, impl):
    """as_text(calls(ns, nc, f64, impl)) and the number of calls."""
    extra = rules(ns, nc, f64, impl)
    text = PRODUCTS.replace("@n", str(ns)).replace("@c", str(nc)).replace("@d", str(f64)).replace("@i", str(impl))
    return text + as_text(extra), N_PRODUCTS + len(extra)


def cells():
    return [(ns, nc, f64, impl) for ns, nc in SHAPES for f64 in (0, 1) for impl in IMPLS]


def build_probe(lib_path, exe):
    """tests/step_route_probe.cpp, built host-only against the library at lib_path (the compiler of csrc/Makefile)."""
    lib_dir = os.path.dirname(os.path.abspath(lib_path))
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-x", "hip", "--cuda-host-only",
                           os.path.join(ROOT, "tests", "step_route_probe.cpp"), "-o", exe, "-L" + lib_dir, "-lmpc_lqr_hip",
                           "-Wl,-rpath," + lib_dir])
    return exe


def lines(exe, text):
    """The probe's line of every call of text (through standard input; the ring switches of the A/B tests out of the way)."""
    env = {k: v for k, v in os.environ.items() if k not in ("MPC_DPP16_RING", "MPC_MFMA40_RING", "MPC_DPP16_RESIDENT")}
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, env=env, check=True).stdout.split(b"\n")[:-1]
    assert len(out) == text.count("\n"), (len(out), text.count("\n"))
    return out


def digests(exe):
    """{"n_state/n_ctrl/f64/impl": sha256 of the cell's lines}, every cell from one run of the probe."""
    per_cell = [(cell,) + cell_text(*cell) for cell in cells()]
    out = lines(exe, "".join(text for _, text, _ in per_cell))
    got, at = {}, 0
    for cell, _, n in per_cell:
        got["%d/%d/%d/%d" % cell] = hashlib.sha256(b"\n".join(out[at:at + n])).hexdigest()
        at += n
    return got


def main():
    import tempfile
    from mpc import _native
    with tempfile.TemporaryDirectory() as tmp:
        got = digests(build_probe(_native.lib_path(), os.path.join(tmp, "step_route_probe")))
    with open(OUT, "w") as fh:
        fh.write('{"calls": %d,\n "cells": {\n' % sum(cell_text(*cell)[1] for cell in cells()))
        fh.write(",\n".join('  "%s": "%s"' % kv for kv in got.items()))
        fh.write("\n }}\n")
    print("%s: %d cells, %d bytes, library %s" % (OUT, len(got), os.path.getsize(OUT), _native.lib_path()))


if __name__ == "__main__":
    main()
