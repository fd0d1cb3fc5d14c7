"""CPU-only: the routing of the KKT backward (csrc/capi.hip: kkt_fused_route, kkt_grads_route; docs/history/r18.md).

1. tests/golden/kkt_route_expect.json, written by hand from the two cascades mpc_lqr_kkt_fused and mpc_lqr_kkt_grads held before
   they were gathered into one decision each, says which fused kernel and which closed-form kernel takes a LEGAL call;
   mpc_lqr_kkt_fused_route and mpc_lqr_kkt_grads_route answer every row, and mpc_lqr_kkt_fused_workspace_bytes the workspace
   beside it.  (tests/test_gpu_kkt_route.py holds the rows torch tensors can express against the kernels themselves.)
2. The six mpc_lqr_kkt_fused calls whose refusals tests/golden/step_route_answers.json recorded from a build before
   docs/history/r15.md: the entry still refuses them with that code and text (tests/test_step_route_host.py), and the query gives
   the same code and text -- except where the entry's reason is "no fused kernel takes this": MPC_KKT_NONE.

No call here reaches a launch; every pointer is made up (the queries dereference none)."""
import ctypes
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN
from mpc import _native

_spec = importlib.util.spec_from_file_location("make_golden_step_route", os.path.join(GOLDEN, "make_golden_step_route.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

KKT = dict(NONE=_native.KKT_NONE, DPP16=_native.KKT_DPP16, DPP16_PAD=_native.KKT_DPP16_PAD, MFMA40=_native.KKT_MFMA40,
           MFMA40_PAD16=_native.KKT_MFMA40_PAD16, MFMA40_PAD4=_native.KKT_MFMA40_PAD4)
GRADS = dict(DPP16=_native.KKT_GRADS_DPP16, WAVE=_native.KKT_GRADS_WAVE, GENERIC=_native.KKT_GRADS_GENERIC)
E_DIMS, E_NULL = -1, -2                      # include/mpc_lqr.h


def expected_routes():
    with open(os.path.join(GOLDEN, "kkt_route_expect.json")) as fh:
        t = json.load(fh)
    return [dict(t["defaults"], **row) for row in t["rows"]]


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def test_the_codes_are_the_headers():
    import re
    with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "mpc_lqr.h")) as fh:
        header = fh.read()
    declared = {name: int(value) for name, value in re.findall(r"\bMPC_KKT_(?!SHARED)([A-Z0-9_]+) = (\d+)", header)}
    assert declared == dict(KKT, **{"GRADS_" + k: v for k, v in GRADS.items()})


def route_arguments(row):
    """The made-up calls of one row -> (p, o, the eleven pointers of mpc_lqr_kkt_fused behind o, bytes, the nine of mpc_lqr_kkt_grads
    behind p, keep)."""
    ns, nc = row["shape"]
    T, B = row["T"], row["B"]
    at = lambda name, base=gen.PTR: base + row["off"].get(name, 0)
    p = gen.problem(_native, ns, nc, _native.MPC_F32 if row["dtype"] == "f32" else _native.MPC_F64, T, B)
    for name in ("x_init", "C", "c", "F", "f", "cur_x", "cur_u"):
        setattr(p, name, at(name))
    for name, more in row["skew"].items():
        setattr(p, name, getattr(p, name) + more)
    for name, value in row["set"].items():
        setattr(p, name, value)
    if T == 1:
        p.F = None
    o, keep = gen.options(_native, box={"none": 0, "tensor": 2}[row["bounds"]], flags=gen.OPT_C_SYMMETRIC if row["symmetric"] else 0,
                          env=(row["env"], 0) if row["env"] else None)
    if row["bounds"] == "tensor":
        o.lo, o.hi = at("lo"), at("hi")
    many = T > 1
    nbytes = int(_native.load().mpc_lqr_kkt_fused_workspace_bytes(ctypes.byref(p)))
    fused = (at("dl_dx"), at("dl_du"), at("dC"), at("dc"), at("dF") if many else None, at("df") if many else None, at("dx_init"),
             at("dx_out"), at("du_out"), None, at("ws", gen.WS))
    grads = (at("dx"), at("du"), at("dl_dx"), at("dl_du"), at("dC"), at("dc"), at("dF") if many else None, at("df") if many else None,
             at("dx_init"))
    return p, o, fused, nbytes, grads, keep


@pytest.mark.parametrize("row", expected_routes(), ids=lambda row: row["id"])
def test_a_legal_backward_takes_the_kernels_the_cascades_gave_it(row, lib):
    p, o, fused, nbytes, grads, _keep = route_arguments(row)
    r = ctypes.byref
    assert nbytes == 4 * row["T"] * row["B"] * row["ws_floats"] + 64
    kernel = int(lib.mpc_lqr_kkt_fused_route(r(p), r(o), *fused, nbytes))
    assert kernel >= 0, lib.mpc_lqr_last_error().decode()
    assert kernel == KKT[row["kernel"]]
    # the supported query is the route's answer on sizes, dtype and flags alone: 0 exactly where no alignment could help
    none_at_all = row["kernel"] == "NONE" and not (set(row["off"]) & {"ws", "lo", "hi"})
    assert int(lib.mpc_lqr_kkt_fused_supported(r(p), r(o))) == (0 if none_at_all else 1)
    kernel = int(lib.mpc_lqr_kkt_grads_route(r(p), *grads))
    assert kernel > 0, lib.mpc_lqr_last_error().decode()
    assert kernel == GRADS[row["grads"]]


def test_an_empty_batch_launches_nothing(lib):
    p, o, fused, nbytes, grads, _keep = route_arguments(expected_routes()[0])
    p.B = 0
    assert int(lib.mpc_lqr_kkt_fused_route(ctypes.byref(p), ctypes.byref(o), *fused, nbytes)) == 0
    assert int(lib.mpc_lqr_kkt_grads_route(ctypes.byref(p), *grads)) == 0


def test_the_closed_form_query_refuses_what_its_entry_refuses(lib):
    p, _o, _fused, _nbytes, grads, _keep = route_arguments(expected_routes()[0])
    r = ctypes.byref
    for i, text in ((0, "kkt_grads: NULL argument"), (5, "kkt_grads: NULL argument"), (6, "kkt_grads: dF is NULL")):
        args = grads[:i] + (None,) + grads[i + 1:]
        assert int(lib.mpc_lqr_kkt_grads(r(p), *args, None)) == E_NULL and lib.mpc_lqr_last_error().decode() == text
        assert int(lib.mpc_lqr_kkt_grads_route(r(p), *args)) == E_NULL and lib.mpc_lqr_last_error().decode() == text
    p.nc = 65
    assert int(lib.mpc_lqr_kkt_grads_route(r(p), *grads)) == E_DIMS == int(lib.mpc_lqr_kkt_grads(r(p), *grads, None))


def test_the_fused_query_refuses_what_its_entry_refuses():
    """The six refused mpc_lqr_kkt_fused calls of step_route_answers.json, built as its generator builds them.  Where a fused kernel
    covers the shape (the recorded mpc_lqr_kkt_fused_supported under MPC_OPT_C_SYMMETRIC), kkt_not_symmetric and kkt_misaligned are
    legal calls no fused kernel takes -- MPC_KKT_NONE -- and the other four give the entry's code and text.  Where none does
    (float64, beyond 32/8) the entry refuses all six with that reason before it looks at anything else, and so all six are NONE."""
    with open(os.path.join(GOLDEN, "step_route_answers.json")) as fh:
        table = gen.unpack(json.load(fh))
    L = _native.load()
    r = ctypes.byref
    no_kernel = "mpc_lqr_kkt_fused: needs fp32"
    for want in table:
        ns, nc, dtype = want["n_state"], want["n_ctrl"], want["dtype"]
        p, nof = gen.problem(_native, ns, nc, dtype, 5, 3), gen.problem(_native, ns, nc, dtype, 5, 3, f=False)
        plain, _ = gen.options(_native)
        sym, _ = gen.options(_native, flags=gen.OPT_C_SYMMETRIC)
        kfull = int(L.mpc_lqr_kkt_fused_workspace_bytes(r(p)))
        grads = (gen.PTR,) * 9
        calls = {"kkt_df_without_f": (r(nof), r(sym), *grads, None, gen.WS, kfull),
                 "kkt_not_symmetric": (r(p), r(plain), *grads, None, gen.WS, kfull),
                 "kkt_nows": (r(p), r(sym), *grads, None, None, 0),
                 "kkt_short": (r(p), r(sym), *grads, None, gen.WS, 16),
                 "kkt_misaligned": (r(p), r(sym), *grads, None, gen.WS + 4, kfull),
                 "kkt_dx_without_du": (r(p), r(sym), *grads[:8], None, None, gen.WS, kfull)}
        covered = want["kkt_fused_supported"]["symmetric"] == 1
        for variant, args in calls.items():
            code, text = want["refusals"][variant]
            assert [int(L.mpc_lqr_kkt_fused(*args, None)), L.mpc_lqr_last_error().decode()] == [code, text], (ns, nc, dtype, variant)
            got = int(L.mpc_lqr_kkt_fused_route(*args))
            if variant in ("kkt_not_symmetric", "kkt_misaligned") or not covered:
                assert code == E_DIMS and (text.startswith(no_kernel) or variant == "kkt_misaligned")
                assert got == _native.KKT_NONE, (ns, nc, dtype, variant, got)
            else:
                assert [got, L.mpc_lqr_last_error().decode()] == [code, text], (ns, nc, dtype, variant)
