"""CPU-only: the routing of the step entry (csrc/capi.hip: step_route) answers what the ladder of step_impl and its mirrors
answered before they were gathered into one decision (docs/history/r15.md).

1. tests/golden/step_route_answers.json was recorded from a build of the commit before that change by
   tests/golden/make_golden_step_route.py; every row is recomputed here, by the generator's own probing code, on the library under
   test and compared exactly: mpc_lqr_impl_supported, mpc_lqr_workspace_bytes, mpc_lqr_qp_record, the fused KKT backward's two
   queries, and the code and text with which mpc_lqr_step / _sweep / _rollout / _kkt_fused refuse a call before any launch.
2. mpc_lqr_step_route refuses each of those mpc_lqr_step calls with the same code and text.
3. tests/golden/step_route_expect.json, written by hand from that ladder, says which kernel (and sweep ring) takes a LEGAL call;
   mpc_lqr_step_route answers every row.  (tests/test_gpu_step_route.py holds the same table against the kernels themselves;
   the exact and the padded instantiation of one kernel may produce the same bits at the exact shape, so that pair is
   told apart here alone.)

No call here reaches a launch; every pointer is made up (mpc_lqr_step_route dereferences none)."""
import ctypes
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN
from mpc import _native



def _generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


gen = _generator("make_golden_step_route")
full = _generator("make_golden_step_route_full")


def expected_routes():
    with open(os.path.join(GOLDEN, "step_route_expect.json")) as fh:
        t = json.load(fh)
    return [dict(t["defaults"], **row) for row in t["rows"]]


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "step_route_answers.json")) as fh:
        return gen.unpack(json.load(fh))


@pytest.fixture
def lib(monkeypatch):
    # (the ring switches of the A/B tests: the tables are the library's own choice)
    monkeypatch.delenv("MPC_DPP16_RING", raising=False)
    monkeypatch.delenv("MPC_MFMA40_RING", raising=False)
    _native.load()                               # (checks the ABI and that every declared entry is there)
    L = gen.bind(_native)
    L.mpc_lqr_step_route.argtypes = L.mpc_lqr_step.argtypes[:6] + [ctypes.POINTER(ctypes.c_int)]
    return L


def test_the_table_covers_the_shapes_and_both_dtypes(table):
    assert [(r["n_state"], r["n_ctrl"], r["dtype"]) for r in table] == \
        [(ns, nc, d) for ns, nc in gen.SHAPES for d in (_native.MPC_F32, _native.MPC_F64)]
    by = {(r["n_state"], r["n_ctrl"], r["dtype"]): r for r in table}
    # a few cells as the library answered them before the change: the 12/4 query looks at sizes alone, the padded one at the options
    assert by[(12, 4, 0)]["impl_supported"]["ls17"][0] == "010100000" and by[(12, 4, 0)]["impl_supported"]["ls16"][0] == "011100011"
    assert by[(32, 8, 0)]["workspace_bytes"][1] == 5 * 3 * 632 * 4 + 3 * 4 + 256
    assert by[(12, 4, 0)]["qp_record"]["aligned"]["box1"][0] == [1, 192, 192, 64]
    assert by[(12, 4, 0)]["qp_record"]["pointers+4"]["box1"][0][0] == 0
    assert all(len(r["refusals"]) > 40 for r in table)


def test_every_answer_is_the_recorded_one(table, lib):
    for want in table:
        got = gen.answers(_native, lib, want["n_state"], want["n_ctrl"], want["dtype"])
        assert got.keys() == want.keys()
        for key in want:
            if key != "refusals":
                assert got[key] == want[key], (want["n_state"], want["n_ctrl"], want["dtype"], key, got[key], want[key])
        assert got["refusals"].keys() == want["refusals"].keys()
        for variant, w in want["refusals"].items():
            assert got["refusals"][variant] == w, (want["n_state"], want["n_ctrl"], want["dtype"], variant, got["refusals"][variant], w)


def test_the_route_query_refuses_what_the_step_refuses(table, lib):
    r = ctypes.byref
    for want in table:
        for variant, (p, o, out, ws, nbytes, impl) in gen.step_calls(_native, lib, want["n_state"], want["n_ctrl"], want["dtype"]):
            ring = ctypes.c_int(-1)
            rc = int(lib.mpc_lqr_step_route(r(p), r(o), r(out), ws, nbytes, impl, r(ring)))
            assert [rc, lib.mpc_lqr_last_error().decode()] == want["refusals"][variant], (want["n_state"], want["n_ctrl"], want["dtype"], variant)


def route_arguments(row):
    """The made-up call of one row of step_route_expect.json -> (p, o, out, workspace, bytes, keep)."""
    ns, nc = row["shape"]
    dtype = _native.MPC_F32 if row["dtype"] == "f32" else _native.MPC_F64
    p = gen.problem(_native, ns, nc, dtype, row["T"], row["B"], ptr=gen.PTR + (0 if row["align"] == 16 else 4))
    o, keep = gen.options(_native, box={"none": 0, "scalar": 1, "tensor": 2}[row["bounds"]], max_ls=row["max_ls"],
                          flags=gen.OPT_SWEEP_ONLY if row["sweep_only"] else 0)
    if row["mask"]:
        o.zero_mask = gen.PTR
    out = gen.outputs(_native, gains=row["gains"])
    full = int(_native.load().mpc_lqr_workspace_bytes(ctypes.byref(p)))
    ws, nbytes = {"full": (gen.WS, full), "misaligned": (gen.WS + 4, full), "none": (None, 0)}[row["workspace"]]
    return p, o, out, ws, nbytes, keep


@pytest.mark.parametrize("row", expected_routes(), ids=lambda row: row["id"])
def test_a_legal_call_takes_the_kernel_the_ladder_gave_it(row, lib):
    p, o, out, ws, nbytes, _keep = route_arguments(row)
    ring = ctypes.c_int(-1)
    r = ctypes.byref
    kernel = int(lib.mpc_lqr_step_route(r(p), r(o), r(out), ws, nbytes, row["impl"], r(ring)))
    assert kernel > 0, lib.mpc_lqr_last_error().decode()
    assert (kernel, ring.value) == (row["kernel"], row["ring"])
    assert int(lib.mpc_lqr_step_route(r(p), r(o), r(out), ws, nbytes, row["impl"], None)) == kernel       # ring may be NULL


def test_the_route_follows_the_ring_switches(lib, monkeypatch):
    """MPC_DPP16_RING / MPC_MFMA40_RING force a ring; the suite runs with MPC_DPP16_RING_DYNAMIC, so the route re-reads them."""
    rows = {row["id"]: row for row in expected_routes()}
    r = ctypes.byref
    for name, var, forced in (("12/4 box, small batch: deep ring", "MPC_DPP16_RING", 2), ("12/4 unconstrained: short ring", "MPC_DPP16_RING", 4),
                              ("32/8 unconstrained, small batch: three slots", "MPC_MFMA40_RING", 2)):
        p, o, out, ws, nbytes, _keep = route_arguments(rows[name])
        monkeypatch.setenv(var, str(forced))
        ring = ctypes.c_int(-1)
        assert int(lib.mpc_lqr_step_route(r(p), r(o), r(out), ws, nbytes, 0, r(ring))) == rows[name]["kernel"]
        assert ring.value == forced
        monkeypatch.delenv(var)


def test_an_empty_batch_launches_nothing(lib):
    p, o, out, ws, nbytes, _keep = route_arguments(expected_routes()[0])
    p.B = 0
    assert int(lib.mpc_lqr_step_route(ctypes.byref(p), ctypes.byref(o), ctypes.byref(out), ws, nbytes, 0, None)) == 0


# ---------------------------------------------------------------------------------------------
# the whole StepRoute, not only (kernel, ring): what step_impl patches its launch from
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/step_route_probe.cpp, built host-only against the library under test (the compiler of csrc/Makefile)."""
    import subprocess
    exe = full.build_probe(_native.lib_path(), str(tmp_path_factory.mktemp("probe") / "step_route_probe"))

    def run(*calls):
        env = dict(os.environ)
        env.pop("MPC_DPP16_RING", None)
        env.pop("MPC_MFMA40_RING", None)
        out = subprocess.check_output([exe] + [str(v) for call in calls for v in call], env=env).decode()
        return [json.loads(line) for line in out.splitlines()]
    run.exe = exe
    return run


def test_the_route_puts_every_piece_where_the_ladder_put_it(probe):
    """[T,B] = [5,3], so T B = 15.  The expected offsets are the literals of step_impl / status_scratch_offset / mpc_lqr_qp_record as they
    stood before docs/history/r15.md: fused records T B (128 + 16) floats at 0; 32/8: K [T,B,8,32] | k [T,B,8] | (M, Quu, m) + second
    trial T B (328 + 40) floats, the record only in the constrained modes and with the room; padded 32/8: the same on the kernel's own
    padded gains; generic: K | k; the parked status words behind the largest of them, rounded to 16."""
    NONE, SCALAR = 0, 1
    FULL, NO_WS, GAINS_ONLY = 1, 0, 3
    #        ns  nc f64 T  B  bounds  mask ls sweep gains ws     align impl status  (+ no simulator, the whole step)
    calls = {
        "12/4 box": (12, 4, 0, 5, 3, SCALAR, 0, 10, 0, 0, FULL, 16, 0, 0),
        "12/4 box off the grid": (12, 4, 0, 5, 3, SCALAR, 0, 10, 0, 0, FULL, 4, 0, 1),
        "32/8 box": (32, 8, 0, 5, 3, SCALAR, 0, 10, 0, 0, FULL, 16, 0, 1),
        "32/8 box, room for the gains only": (32, 8, 0, 5, 3, SCALAR, 0, 10, 0, 0, GAINS_ONLY, 16, 0, 1),
        "32/8 unconstrained": (32, 8, 0, 5, 3, NONE, 0, 10, 0, 0, FULL, 16, 0, 1),
        "32/8 box, gains given": (32, 8, 0, 5, 3, SCALAR, 0, 10, 0, 1, FULL, 16, 0, 1),
        "32/8 box, gains given, no workspace": (32, 8, 0, 5, 3, SCALAR, 0, 10, 0, 1, NO_WS, 16, 0, 1),
        "13/4 gains given": (13, 4, 0, 5, 3, NONE, 0, 10, 0, 1, FULL, 16, 0, 1),
        "16/4": (16, 4, 0, 5, 3, NONE, 0, 10, 0, 0, FULL, 16, 0, 1),
        "16/4 off the grid": (16, 4, 0, 5, 3, NONE, 0, 10, 0, 0, FULL, 4, 0, 1),
        "3/1": (3, 1, 0, 5, 3, NONE, 0, 10, 0, 0, FULL, 16, 0, 1),
        "3/1 sweep only": (3, 1, 0, 5, 3, NONE, 0, 10, 1, 1, FULL, 16, 0, 1),
        "48/16": (48, 16, 0, 5, 3, NONE, 0, 10, 0, 0, FULL, 16, 0, 0),
        "5/3 float64": (5, 3, 1, 5, 3, NONE, 0, 10, 0, 0, FULL, 16, 0, 0),
        "12/4 forced generic, gains given": (12, 4, 0, 5, 3, NONE, 0, 10, 0, 1, FULL, 16, 1, 1),
    }
    TB = 15
    k40, Kk40, pad = TB * 256 * 4, TB * (256 + 8) * 4, TB * (256 + 8 + 328 + 40) * 4
    base = dict(code=0, phase=3, ring=0, pad16=0, needs_resolve=1, K_off=-1, k_off=-1, Kk_off=-1, status_off=-1, qp=[-1, 0, 0])
    want = {
        "12/4 box": dict(kernel=3, ring=4, Kk_off=0, status_off=pad, qp=[48 * 4, 3 * 64, 64]),
        "12/4 box off the grid": dict(kernel=8, Kk_off=0),
        "32/8 box": dict(kernel=5, ring=3, K_off=0, k_off=k40, Kk_off=Kk40, qp=[k40, 3 * 8, 8]),
        "32/8 box, room for the gains only": dict(kernel=5, ring=3, K_off=0, k_off=k40, qp=[k40, 3 * 8, 8]),
        "32/8 unconstrained": dict(kernel=5, ring=3, K_off=0, k_off=k40, qp=[k40, 3 * 8, 8]),
        "32/8 box, gains given": dict(kernel=5, ring=3, Kk_off=Kk40),
        "32/8 box, gains given, no workspace": dict(kernel=5, ring=3),
        "13/4 gains given": dict(kernel=7, K_off=0, k_off=k40, Kk_off=Kk40, qp=[k40, 3 * 8, 8]),
        "16/4": dict(kernel=7, pad16=1, K_off=0, k_off=k40, Kk_off=Kk40, qp=[k40, 3 * 8, 8]),
        "16/4 off the grid": dict(kernel=7, pad16=0, K_off=0, k_off=k40, Kk_off=Kk40, qp=[k40, 3 * 8, 8]),
        "3/1": dict(kernel=6, needs_resolve=0, Kk_off=0),
        "3/1 sweep only": dict(kernel=1, phase=1, needs_resolve=0),
        "48/16": dict(kernel=1, needs_resolve=0, K_off=0, k_off=TB * 16 * 48 * 4, status_off=TB * (16 * 48 + 16) * 4),
        "5/3 float64": dict(kernel=2, Kk_off=0, status_off=TB * (128 + 16) * 4),
        "12/4 forced generic, gains given": dict(kernel=1, needs_resolve=0),
    }
    got = probe(*(call + (0, 0, 0, 3) for call in calls.values()))
    assert len(got) == len(calls)
    for name, g in zip(calls, got):
        assert g.pop("msg") is None and g.pop("entry") == [want[name]["kernel"], want[name].get("ring", 0), ""]
        assert g.pop("workspace_bytes") == _native.load().mpc_lqr_workspace_bytes(ctypes.byref(gen.problem(_native, *calls[name][:2], calls[name][2], 5, 3)))
        assert g == dict(base, **want[name]), (name, g)


def test_the_whole_route_is_the_one_before_the_kernels_became_a_table(probe, tmp_path):
    """tests/golden/step_route_full.json: one digest per (shape, dtype, impl) over the probe's lines of the grid of
    make_golden_step_route_full.py -- simulators, gains, workspaces, bounds, masks, alignments, the batch rules, the two phases --,
    recorded from a build of the commit before docs/history/r22.md.  A cell that differs is run again and shown; with
    MPC_LQR_HIP_PARENT_LIB pointing at a build of that commit, next to that build's lines from the first call that differs."""
    with open(os.path.join(GOLDEN, "step_route_full.json")) as fh:
        want = json.load(fh)["cells"]
    got = full.digests(probe.exe)
    assert list(got) == list(want)
    bad = [cell for cell in got if got[cell] != want[cell]]
    if bad:
        cs = full.calls(*(int(v) for v in bad[0].split("/")))
        mine = full.lines(probe.exe, full.as_text(cs))
        shown = ["%d cells differ: %s" % (len(bad), " ".join(bad)), "cell %s:" % bad[0]]
        parent = os.environ.get("MPC_LQR_HIP_PARENT_LIB")
        if parent:
            theirs = full.lines(full.build_probe(parent, str(tmp_path / "parent_probe")), full.as_text(cs))
            i = next((i for i in range(len(cs)) if mine[i] != theirs[i]), None)
            shown += ["no line differs from that build's: the table was not recorded from it"] if i is None else \
                     ["call %d %r" % (i, cs[i]), "  here:   " + mine[i].decode(), "  parent: " + theirs[i].decode()]
        else:
            shown += ["%r -> %s" % (c, line.decode()) for c, line in zip(cs, mine)]
        pytest.fail("\n".join(shown))


def test_the_record_query_answers_for_the_kernel_that_takes_the_call(lib):
    """mpc_lqr_qp_record where the recorded table has no row: a 32/8 float32 call that box and mask together, or more than sixteen
    line-search trials, send to the generic kernels keeps no record (they ignore the hint); the commit before docs/history/r15.md
    answered those from the sizes alone, under impl 0 and under a forced impl 5 (a step the library refuses)."""
    r = ctypes.byref
    p = gen.problem(_native, 32, 8, _native.MPC_F32, 5, 3)
    for box, mask, max_ls, want in ((1, False, 10, 1), (1, False, 16, 1), (1, True, 10, 0), (1, False, 17, 0), (2, True, 17, 0)):
        o, _ = gen.options(_native, box=box, max_ls=max_ls)
        if mask:
            o.zero_mask = gen.PTR
        for impl in (0, 5):
            off, st, sb = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
            assert int(lib.mpc_lqr_qp_record(r(p), r(o), impl, r(off), r(st), r(sb))) == want, (box, mask, max_ls, impl)
            assert (off.value, st.value, sb.value) == ((5 * 3 * 256 * 4, 3 * 8, 8) if want else (-7, -7, -7))
