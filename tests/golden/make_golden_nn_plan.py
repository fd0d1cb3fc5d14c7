"""What the host side of the NNDynamics kernels answers WITHOUT a device: workspace sizes, mpc_mlp_supported, and the
code + mpc_lqr_last_error() text of every entry point for a description it refuses before any launch.

The table (nn_plan_answers.json) is recorded from a build of the commit BEFORE the host code was rewritten around one
layout / one validation / one plan (docs/history/r13.md): build that commit somewhere, then

    MPC_LQR_HIP_LIB=/path/to/that/libmpc_lqr_hip.so python tests/golden/make_golden_nn_plan.py

tests/test_nn_plan_host.py recomputes every row with `answers()` below on the library under test and compares exactly.

No recorded call may reach a kernel launch (there is no device here, and what happens then is not contract).  So every
call of the error table is refused BY CONSTRUCTION, whatever else the description is:

  probe       widths alone (activation 0, W / b NULL), a plausible workspace: stops at the NULL weights at the latest
  carry       complete, ctrl_carry = n_ctrl: the linearisations and the weight gradient refuse that first; the rollout,
              which takes it, gets no workspace
  act<a>      complete, activation a in {-1, 0, 1, 2, 3}, no workspace (the weight gradient: a workspace of 0 bytes,
              its own NULL test comes first otherwise)
  badcarry    complete, ctrl_carry = n_ctrl + 1 (neither 0 nor n_ctrl), a plausible workspace
  dims        complete, called with n_state - 1 (the widths no longer match)
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "mpc.pytorch_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "nn_plan_answers.json")
GRAD_N = (0, 1, 16 * 1024, 10 ** 6)
ENTRIES = ("mpc_mlp_linearize", "mpc_mlp_linearize_carry", "mpc_mlp_rollout", "mpc_mlp_param_grad")
E_LAUNCH = -4
PTR, WS, WS_BYTES = 16, 4096, 1 << 40          # dummy non-NULL pointers: nothing recorded here dereferences one


def descriptions():
    """(n_layers, widths): 0 to 5 layers, the shapes and hidden widths the issue names (the deeper combinations thinned),
    the boundary cases of tests/test_nn_wide_host.py and tests/test_host_logic.py, and a network on each side of every rule:
    register-resident [16,128,12] / not [16,129,12], [17,100,12]; weights staged [16,100,100,12] / from global memory
    [16,256,100,12] (145,920 bytes packed); fits [40,1024,32] (rollout only) / too wide [40,512,512,32];
    gW tiles <= 16 [16,100,12] / > 16 [40,100,32] / > PG_MAX_TILES [16,256,100,12]."""
    shapes = [(4, 1), (12, 4), (12, 5), (16, 8), (17, 3), (28, 4), (32, 8), (33, 7)]
    hidden = [1, 15, 16, 17, 100, 128, 129, 256, 1024, 4096, 4097]
    rows = [(0, [0, 0]), (5, [16, 8, 8, 8, 8])]            # (five layers: the struct has no sixth width to give)
    for ns, nc in shapes:
        rows.append((1, [ns + nc, ns]))
        for h in (hidden if (ns, nc) in ((4, 1), (12, 4), (32, 8)) else (16, 100, 128, 129, 1024)):
            rows.append((2, [ns + nc, h, ns]))
    pairs = [(100, 100), (256, 100), (300, 300), (512, 512), (16, 17), (1, 4097), (128, 129), (1024, 16), (4096, 15), (15, 1)]
    for (ns, nc), (h1, h2) in itertools.product(((12, 4), (28, 4)), pairs):
        rows.append((3, [ns + nc, h1, h2, ns]))
    for ns, nc in ((4, 1), (12, 4), (32, 8)):
        for hs in ((16, 16, 16), (100, 17, 129), (256, 32, 20), (1024, 1, 15)):
            rows.append((4, [ns + nc] + list(hs) + [ns]))
    named = [[16, 100, 12], [16, 300, 300, 12], [5, 800, 4], [5, 1024, 4], [20, 512, 12], [5, 2048, 4], [40, 100, 32],
             [37, 64, 48, 32], [20, 17], [25, 64, 20], [49, 100, 33], [24, 256, 32, 20, 16], [40, 1024, 32], [40, 512, 512, 32],
             [41, 100, 33], [16, 256, 100, 12], [16, 100, 100, 12], [16, 0, 12], [16, -3, 12], [16, 128, 12], [16, 129, 12]]
    rows += [(len(w) - 1, w) for w in named]
    seen, out = set(), []
    for L, w in rows:
        if (L, tuple(w)) not in seen:
            seen.add((L, tuple(w)))
            out.append((L, w))
    return out


def _net(native, L, widths, act=0, carry=0, complete=False):
    e = native.MlpDynamics()
    e.n_layers, e.activation, e.passthrough, e.ctrl_carry = L, act, 1, carry
    for l, w in enumerate(widths):
        e.widths[l] = w
    if complete:
        for l in range(native.MLP_MAX_LAYERS):
            e.W[l], e.b[l] = PTR, PTR
    return e


def _refusals(native, lib, e, ns, nc, ws, nbytes, grad_ws):
    """[code, text] of the four entry points for a description they must refuse before any launch."""
    p, out, g = native.Problem(), native.Outputs(), native.MlpParamGrads()
    p.B, p.T, p.ns, p.nc, p.dtype, p.x_init, p.cur_u = 8, 2, ns, nc, native.MPC_F32, PTR, PTR
    out.new_x = PTR
    for l in range(native.MLP_MAX_LAYERS):
        g.gW[l], g.gb[l] = PTR, PTR
    r = ctypes.byref
    calls = (lambda: lib.mpc_mlp_linearize(r(e), ns, nc, 8, PTR, PTR, PTR, PTR, ws, nbytes, None),
             lambda: lib.mpc_mlp_linearize_carry(r(e), ns, nc, 8, PTR, PTR, PTR, PTR, ws, nbytes, None),
             lambda: lib.mpc_mlp_rollout(r(p), None, r(e), None, None, None, r(out), ws, nbytes, None),
             lambda: lib.mpc_mlp_param_grad(r(e), ns, nc, 8, PTR, PTR, PTR, PTR, r(g), grad_ws, nbytes, None))
    got = []
    for name, call in zip(ENTRIES, calls):
        rc = int(call())
        text = lib.mpc_lqr_last_error().decode()
        assert rc not in (0, E_LAUNCH), "%s was meant to be refused before any launch: %d %s" % (name, rc, text)
        got.append([rc, text])
    return got


def answers(native, lib, L, widths):
    """One row of the table, from the library `lib` (mpc._native as `native` for the structs)."""
    ns = widths[L] if 1 <= L <= native.MLP_MAX_LAYERS else widths[-1]
    nc = widths[0] - ns
    row = {"n_layers": L, "widths": widths, "n_state": ns, "n_ctrl": nc}
    probe = _net(native, L, widths)
    row["workspace_bytes"] = int(lib.mpc_mlp_workspace_bytes(ctypes.byref(probe)))
    row["supported_by_widths"] = int(lib.mpc_mlp_supported(ctypes.byref(probe), ns, nc))
    row["complete"] = []                                  # [activation, ctrl_carry, mpc_mlp_supported, grad workspace at GRAD_N]
    for act, carry in itertools.product((0, 1, 2), sorted({0, nc})):
        e = _net(native, L, widths, act, carry, complete=True)
        row["complete"].append([act, carry, int(lib.mpc_mlp_supported(ctypes.byref(e), ns, nc)),
                                [int(lib.mpc_mlp_param_grad_workspace_bytes(ctypes.byref(e), N)) for N in GRAD_N]])
    ref = {"probe": _refusals(native, lib, probe, ns, nc, WS, WS_BYTES, WS)}
    if nc != 0:
        ref["carry"] = _refusals(native, lib, _net(native, L, widths, 0, nc, complete=True), ns, nc, None, 0, WS)
        ref["badcarry"] = _refusals(native, lib, _net(native, L, widths, 0, nc + 1, complete=True), ns, nc, WS, WS_BYTES, WS)
    for act in (-1, 0, 1, 2, 3):
        ref["act%d" % act] = _refusals(native, lib, _net(native, L, widths, act, 0, complete=True), ns, nc, None, 0, WS)
    ref["dims"] = _refusals(native, lib, _net(native, L, widths, 0, 0, complete=True), ns - 1, nc, WS, WS_BYTES, WS)
    row["refusals"] = ref
    return row


def pack(rows):
    """The texts once, the rows referring to them by index: the table stays tens of kilobytes."""
    texts = sorted({t for row in rows for calls in row["refusals"].values() for _, t in calls})
    for row in rows:
        row["refusals"] = {k: [[rc, texts.index(t)] for rc, t in calls] for k, calls in row["refusals"].items()}
    return {"grad_N": list(GRAD_N), "entries": list(ENTRIES), "texts": texts, "rows": rows}


def unpack(table):
    for row in table["rows"]:
        row["refusals"] = {k: [[rc, table["texts"][i]] for rc, i in calls] for k, calls in row["refusals"].items()}
    return table["rows"]


def main():
    from mpc import _native
    lib = _native.load()
    table = pack([answers(_native, lib, L, w) for L, w in descriptions()])
    with open(OUT, "w") as fh:
        fh.write('{"grad_N": %s, "entries": %s,\n "texts": %s,\n "rows": [\n' % tuple(json.dumps(table[k]) for k in ("grad_N", "entries", "texts")))
        fh.write(",\n".join("  " + json.dumps(row, separators=(",", ":")) for row in table["rows"]))
        fh.write("\n ]}\n")
    print("%s: %d rows, %d bytes, library %s" % (OUT, len(table["rows"]), os.path.getsize(OUT), _native.lib_path()))


if __name__ == "__main__":
    main()
