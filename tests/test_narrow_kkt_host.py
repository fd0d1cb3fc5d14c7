"""CPU-only: the fused KKT backward with the kernel named by the caller (csrc/capi.hip: kkt_fused_route_kernel;
docs/history/r19.md) -- mpc_lqr_kkt_fused_kernel_route and mpc_lqr_kkt_fused_kernel_workspace_bytes under kernel = 0 (the existing
entries' answers, row by row of the two recorded tables), under MPC_KKT_PREFER_NARROW and under exact codes -- and the flags
`LQRStep(narrow_kkt_kernel=True)` / `mpc.MPC(narrow_kkt_kernel=True)` on a spying stand-in backend.

No call here reaches a launch; every pointer of the C calls is made up (the queries dereference none)."""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN
from mpc import _native, mpc
from mpc.lqr_step import LQRStep
from mpc.mpc import LinDx, QuadCost
from oracle_backend import OracleBackend

_spec = importlib.util.spec_from_file_location("make_golden_step_route", os.path.join(GOLDEN, "make_golden_step_route.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
r = ctypes.byref
E_DIMS, E_NULL, E_ARG = -1, -2, -5                      # include/mpc_lqr.h
NARROW16, NARROW4, PREFER = 6, 7, 100
NARROW_FLOATS = 448                                     # K 128 | k 8 | V 256 | v,g 32 | dx 16 | du 8


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def test_the_python_constants_are_the_c_ones(lib):
    import re
    with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "mpc_lqr.h")) as fh:
        header = fh.read()
    declared = {name: int(value) for name, value in re.findall(r"#define MPC_KKT_(MFMA40_NARROW16|MFMA40_NARROW4|PREFER_NARROW) (\d+)", header)}
    assert declared == dict(MFMA40_NARROW16=_native.KKT_MFMA40_NARROW16, MFMA40_NARROW4=_native.KKT_MFMA40_NARROW4,
                            PREFER_NARROW=_native.KKT_PREFER_NARROW)
    assert (_native.KKT_MFMA40_NARROW16, _native.KKT_MFMA40_NARROW4, _native.KKT_PREFER_NARROW) == (NARROW16, NARROW4, PREFER)
    assert int(lib.mpc_lqr_abi_version()) == 9
    codes = {name: int(value) for name, value in re.findall(r"\bMPC_E_([A-Z]+) = (-\d+)", header)}
    assert (codes["DIMS"], codes["NULL"], codes["ARG"]) == (E_DIMS, E_NULL, E_ARG)


# ---------------------------------------------------------------------------------------------
# kernel = 0: the existing entries, row by row
# ---------------------------------------------------------------------------------------------
def expected_routes():
    with open(os.path.join(GOLDEN, "kkt_route_expect.json")) as fh:
        t = json.load(fh)
    return [dict(t["defaults"], **row) for row in t["rows"]]


def route_arguments(row):
    """tests/test_kkt_route_host.py's made-up call of one row -> (p, o, the eleven pointers behind o, bytes, keep)"""
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
    nbytes = int(_native.load().mpc_lqr_kkt_fused_workspace_bytes(r(p)))
    fused = (at("dl_dx"), at("dl_du"), at("dC"), at("dc"), at("dF") if many else None, at("df") if many else None, at("dx_init"),
             at("dx_out"), at("du_out"), None, at("ws", gen.WS))
    return p, o, fused, nbytes, keep


@pytest.mark.parametrize("row", expected_routes(), ids=lambda row: row["id"])
def test_kernel_0_answers_every_recorded_route_as_the_existing_entry(row, lib):
    p, o, fused, nbytes, _keep = route_arguments(row)
    assert int(lib.mpc_lqr_kkt_fused_kernel_workspace_bytes(r(p), r(o), 0)) == nbytes == 4 * row["T"] * row["B"] * row["ws_floats"] + 64
    assert int(lib.mpc_lqr_kkt_fused_kernel_workspace_bytes(r(p), None, 0)) == nbytes
    old = int(lib.mpc_lqr_kkt_fused_route(r(p), r(o), *fused, nbytes))
    assert old >= 0
    assert int(lib.mpc_lqr_kkt_fused_kernel_route(r(p), r(o), 0, *fused, nbytes)) == old
    # ... and auto never proposes a forced-only kernel
    assert old not in (NARROW16, NARROW4)


def test_kernel_0_refuses_the_six_recorded_calls_as_the_existing_entries(lib):
    """the six refused mpc_lqr_kkt_fused calls per shape of step_route_answers.json (tests/test_kkt_route_host.py builds them so):
    the new entry and the new query under kernel = 0 give the recorded code and text, the query MPC_KKT_NONE where the old query does"""
    with open(os.path.join(GOLDEN, "step_route_answers.json")) as fh:
        table = gen.unpack(json.load(fh))
    L = lib
    for want in table:
        ns, nc, dtype = want["n_state"], want["n_ctrl"], want["dtype"]
        p, nof = gen.problem(_native, ns, nc, dtype, 5, 3), gen.problem(_native, ns, nc, dtype, 5, 3, f=False)
        plain, _ = gen.options(_native)
        sym, _ = gen.options(_native, flags=gen.OPT_C_SYMMETRIC)
        kfull = int(L.mpc_lqr_kkt_fused_workspace_bytes(r(p)))
        assert int(L.mpc_lqr_kkt_fused_kernel_workspace_bytes(r(p), r(sym), 0)) == kfull
        grads = (gen.PTR,) * 9
        calls = {"kkt_df_without_f": (r(nof), r(sym), grads + (None, gen.WS, kfull)),
                 "kkt_not_symmetric": (r(p), r(plain), grads + (None, gen.WS, kfull)),
                 "kkt_nows": (r(p), r(sym), grads + (None, None, 0)),
                 "kkt_short": (r(p), r(sym), grads + (None, gen.WS, 16)),
                 "kkt_misaligned": (r(p), r(sym), grads + (None, gen.WS + 4, kfull)),
                 "kkt_dx_without_du": (r(p), r(sym), grads[:8] + (None, None, gen.WS, kfull))}
        for variant, (pp, oo, rest) in calls.items():
            code, text = want["refusals"][variant]
            assert [int(L.mpc_lqr_kkt_fused_kernel(pp, oo, 0, *rest, None)), L.mpc_lqr_last_error().decode()] == [code, text], (ns, nc, dtype, variant)
            old = int(L.mpc_lqr_kkt_fused_route(pp, oo, *rest))
            old_text = L.mpc_lqr_last_error().decode()
            assert [int(L.mpc_lqr_kkt_fused_kernel_route(pp, oo, 0, *rest)), L.mpc_lqr_last_error().decode()] == [old, old_text], (ns, nc, dtype, variant)


# ---------------------------------------------------------------------------------------------
# MPC_KKT_PREFER_NARROW and exact codes
# ---------------------------------------------------------------------------------------------
def ask(L, ns, nc, kernel, dtype=None, symmetric=True, env=None, box=0, off=None, set_=None, T=5, B=3, short=0, ws_off=0, entry=False):
    """The route (entry: mpc_lqr_kkt_fused_kernel itself, for calls it refuses) of a made-up call in a workspace of the queried size
    -> (answer, text, the queried bytes)"""
    off = off or {}
    p = gen.problem(_native, ns, nc, _native.MPC_F32 if dtype is None else dtype, T, B)
    for name, more in off.items():
        if hasattr(p, name):
            setattr(p, name, getattr(p, name) + more)
    for name, value in (set_ or {}).items():
        setattr(p, name, value)
    o, keep = gen.options(_native, box=box, flags=gen.OPT_C_SYMMETRIC if symmetric else 0, env=env)
    nbytes = int(L.mpc_lqr_kkt_fused_kernel_workspace_bytes(r(p), r(o), kernel))
    ptrs = (gen.PTR,) * 9 if T > 1 else (gen.PTR,) * 4 + (None, None) + (gen.PTR,) * 3          # (dF, df: T > 1)
    args = (r(p), r(o), kernel) + ptrs + (None, gen.WS + ws_off, nbytes - short)
    rc = int(L.mpc_lqr_kkt_fused_kernel(*args, None)) if entry else int(L.mpc_lqr_kkt_fused_kernel_route(*args))
    return rc, L.mpc_lqr_last_error().decode(), nbytes


def auto(L, ns, nc, **kw):
    return ask(L, ns, nc, 0, **kw)[0]


def test_prefer_narrow_takes_16_byte_gathers_where_everything_sits_on_16_bytes(lib):
    for ns, nc in ((16, 4), (16, 8), (4, 8), (8, 8)):
        for box in (0, 1, 2):
            rc, _, nbytes = ask(lib, ns, nc, PREFER, box=box)
            assert (rc, nbytes) == (NARROW16, 5 * 3 * NARROW_FLOATS * 4 + 64), (ns, nc, box)
        assert ask(lib, ns, nc, PREFER, T=1)[0] == NARROW16


def test_prefer_narrow_takes_dword_gathers_everywhere_else_in_the_envelope(lib):
    for ns, nc in ((13, 4), (14, 3), (9, 6), (1, 5), (15, 8), (16, 1)):
        rc, _, nbytes = ask(lib, ns, nc, PREFER)
        assert (rc, nbytes) == (NARROW4, 5 * 3 * NARROW_FLOATS * 4 + 64), (ns, nc)
    assert ask(lib, 16, 4, PREFER, off=dict(F=4))[0] == NARROW4
    assert ask(lib, 16, 4, PREFER, off=dict(C=4))[0] == NARROW4
    assert ask(lib, 16, 4, PREFER, set_=dict(C_sb=20 * 20 + 1))[0] == NARROW4          # a pitched C_sb
    assert ask(lib, 16, 4, PREFER, off=dict(F=4), T=1)[0] == NARROW16                  # (T = 1 reads no F)


def test_prefer_narrow_is_auto_up_to_12_4_and_beyond_16_8(lib):
    for ns, nc in ((12, 4), (10, 3), (5, 3), (1, 1), (17, 4), (16, 9), (20, 5), (32, 8), (33, 8)):
        rc, _, nbytes = ask(lib, ns, nc, PREFER)
        want, _, wbytes = ask(lib, ns, nc, 0)
        assert (rc, nbytes) == (want, wbytes), (ns, nc)
        assert rc not in (NARROW16, NARROW4)
    assert auto(lib, 12, 4) == _native.KKT_DPP16 and auto(lib, 17, 4) == _native.KKT_MFMA40_PAD4 and auto(lib, 33, 8) == _native.KKT_NONE


def test_prefer_narrow_is_none_where_no_fused_kernel_is(lib):
    assert ask(lib, 16, 4, PREFER, dtype=_native.MPC_F64)[0] == _native.KKT_NONE
    assert ask(lib, 16, 4, PREFER, symmetric=False)[0] == _native.KKT_NONE
    assert ask(lib, 3, 1, PREFER, env=(1, 0))[0] == _native.KKT_NONE                            # a simulator (the pendulum: 3/1)
    # ... and the entry refuses those as the existing entry does
    for kw in (dict(dtype=_native.MPC_F64), dict(symmetric=False)):
        rc, text, _ = ask(lib, 16, 4, PREFER, entry=True, **kw)
        assert rc == E_DIMS and text.startswith("mpc_lqr_kkt_fused: needs fp32")
    # a workspace nobody can use: legal, no kernel
    assert ask(lib, 16, 4, PREFER, ws_off=4)[0] == _native.KKT_NONE
    rc, text, _ = ask(lib, 16, 4, PREFER, ws_off=4, entry=True)
    assert rc == E_DIMS and "16-byte aligned" in text


def test_an_exact_code_is_that_kernel_or_a_refusal_that_names_it(lib):
    rc, text, _ = ask(lib, 13, 4, NARROW16)
    assert (rc, text) == (E_DIMS, "mpc_lqr_kkt_fused_kernel: MPC_KKT_MFMA40_NARROW16 needs n_state <= 16, n_ctrl <= 8, both multiples of 4")
    assert ask(lib, 13, 4, NARROW16, entry=True)[:2] == (rc, text)
    rc, text, _ = ask(lib, 17, 4, NARROW4)
    assert (rc, text) == (E_DIMS, "mpc_lqr_kkt_fused_kernel: MPC_KKT_MFMA40_NARROW4 needs n_state <= 16, n_ctrl <= 8")
    assert ask(lib, 5, 3, NARROW4)[0] == NARROW4                                       # below 12/4 too, when asked for by code
    assert ask(lib, 12, 4, NARROW16)[0] == NARROW16
    assert ask(lib, 16, 4, NARROW16)[0] == NARROW16 and ask(lib, 16, 4, NARROW4)[0] == NARROW4
    rc, text, _ = ask(lib, 16, 4, NARROW16, off=dict(C=4))
    assert rc == E_DIMS and text.startswith("mpc_lqr_kkt_fused_kernel: MPC_KKT_MFMA40_NARROW16 needs C and F 16-byte aligned")
    assert ask(lib, 16, 4, NARROW4, dtype=_native.MPC_F64)[:2] == (E_DIMS, "mpc_lqr_kkt_fused_kernel: MPC_KKT_MFMA40_NARROW4 needs float32")
    assert ask(lib, 16, 4, NARROW4, symmetric=False)[:2] == (E_DIMS, "mpc_lqr_kkt_fused_kernel: MPC_KKT_MFMA40_NARROW4 needs MPC_OPT_C_SYMMETRIC")
    # the existing kernels by their codes: what auto picks is what its code gives, and a code that does not fit is refused, not replaced
    for ns, nc in ((12, 4), (5, 3), (32, 8), (16, 4), (13, 4)):
        k = auto(lib, ns, nc)
        assert ask(lib, ns, nc, k)[0] == k
    rc, text, _ = ask(lib, 13, 4, _native.KKT_DPP16)
    assert (rc, text) == (E_DIMS, "mpc_lqr_kkt_fused_kernel: MPC_KKT_DPP16 needs n_state = 12, n_ctrl = 4")
    for code in (99, 8, -1, 101):
        rc, text, nbytes = ask(lib, 16, 4, code)
        assert (rc, nbytes) == (E_ARG, 0) and "unknown kernel code" in text, code
        assert ask(lib, 16, 4, code, entry=True)[0] == E_ARG


def test_the_workspace_is_the_chosen_kernels(lib):
    for T, B in ((5, 3), (50, 4096), (1, 1)):
        p = gen.problem(_native, 16, 4, _native.MPC_F32, T, B)
        sym, _ = gen.options(_native, flags=gen.OPT_C_SYMMETRIC)
        narrow = T * B * NARROW_FLOATS * 4 + 64
        wide = int(lib.mpc_lqr_kkt_fused_workspace_bytes(r(p)))
        assert wide == T * B * 1392 * 4 + 64
        for code in (NARROW16, NARROW4, PREFER):
            assert int(lib.mpc_lqr_kkt_fused_kernel_workspace_bytes(r(p), r(sym), code)) == narrow
            assert int(lib.mpc_lqr_kkt_fused_kernel_workspace_bytes(r(p), None, code)) == narrow
        for code in (0, _native.KKT_MFMA40_PAD16, _native.KKT_MFMA40_PAD4):
            assert int(lib.mpc_lqr_kkt_fused_kernel_workspace_bytes(r(p), r(sym), code)) == wide
    # one byte short of the narrow size: the entry's own refusal, for a code and for the family, in the query and in the entry
    for code in (NARROW16, NARROW4, PREFER):
        for entry in (False, True):
            rc, text, _ = ask(lib, 16, 4, code, short=1, entry=entry)
            assert (rc, text) == (E_ARG, "workspace too small (see mpc_lqr_kkt_fused_workspace_bytes)"), (code, entry)
    # ... where the padded kernel under kernel = 0 wants its own, larger one
    p = gen.problem(_native, 16, 4, _native.MPC_F32, 5, 3)
    sym, _ = gen.options(_native, flags=gen.OPT_C_SYMMETRIC)
    args = (gen.PTR,) * 9 + (None, gen.WS, 5 * 3 * NARROW_FLOATS * 4 + 64)
    assert int(lib.mpc_lqr_kkt_fused_kernel_route(r(p), r(sym), 0, *args)) == E_ARG
    assert int(lib.mpc_lqr_kkt_fused_kernel_route(r(p), r(sym), PREFER, *args)) == NARROW16


def test_the_shared_checks_come_first_with_their_texts(lib):
    p = gen.problem(_native, 16, 4, _native.MPC_F32, 5, 3)
    nof = gen.problem(_native, 16, 4, _native.MPC_F32, 5, 3, f=False)
    sym, _ = gen.options(_native, flags=gen.OPT_C_SYMMETRIC)
    nbytes = 5 * 3 * NARROW_FLOATS * 4 + 64
    ptrs = (gen.PTR,) * 9
    for code in (NARROW4, PREFER):
        for args, want in (((r(p), r(sym), code, None) + ptrs[1:] + (None, gen.WS, nbytes), (E_NULL, "kkt_fused: NULL argument")),
                           ((r(p), r(sym), code) + ptrs[:4] + (None,) + ptrs[5:] + (None, gen.WS, nbytes), (E_NULL, "kkt_fused: dF is NULL")),
                           ((r(nof), r(sym), code) + ptrs + (None, gen.WS, nbytes), (E_NULL, "kkt_fused: df goes with f")),
                           ((r(p), r(sym), code) + ptrs[:8] + (None, None, gen.WS, nbytes),
                            (E_NULL, "kkt_fused: pass both dx_out and du_out, or neither")),
                           ((r(p), r(sym), code) + ptrs + (None, None, 0), (E_ARG, "workspace too small (see mpc_lqr_kkt_fused_workspace_bytes)"))):
            assert (int(lib.mpc_lqr_kkt_fused_kernel_route(*args)), lib.mpc_lqr_last_error().decode()) == want, (code, want)
            assert (int(lib.mpc_lqr_kkt_fused_kernel(*args, None)), lib.mpc_lqr_last_error().decode()) == want, (code, want)
        p0 = gen.problem(_native, 16, 4, _native.MPC_F32, 5, 0)
        assert int(lib.mpc_lqr_kkt_fused_kernel(r(p0), r(sym), code, *ptrs, None, gen.WS, nbytes, None)) == 0      # an empty batch
        assert int(lib.mpc_lqr_kkt_fused_kernel_route(r(p0), r(sym), code, *ptrs, None, gen.WS, nbytes)) == 0


# ---------------------------------------------------------------------------------------------
# the flags, on a stand-in backend that records what the backward is handed
# ---------------------------------------------------------------------------------------------
class SpyBackend(OracleBackend):
    """asym: every planned step reports MPC_ST_C_ASYMMETRIC (8) on problem 0, as the kernels do for a C that is not symmetric"""

    def __init__(self, asym=False):
        super().__init__()
        self.asym, self.backwards = asym, []

    def plan_step(self, x_init, C, c, F, f, cur_x, cur_u, opts, impl=0, **kw):
        run = super().plan_step(x_init, C, c, F, f, cur_x, cur_u, opts, impl=impl, **kw)

        def flagged():
            res = run()
            if self.asym:
                res["status"] = res["status"].clone()
                res["status"][0] |= 8
            return res
        return flagged

    def kkt_backward(self, C, c, F, f, x_star, u_star, dl_dx, dl_du, opts, impl=0, **kw):
        self.backwards.append((x_star.shape[2], u_star.shape[2], bool(opts.c_symmetric), dict(kw)))
        return super().kkt_backward(C, c, F, f, x_star, u_star, dl_dx, dl_du, opts, impl=impl)


def problem(ns, nc, T=4, B=2):
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    n = ns + nc
    L = rn(T, B, n, n)
    C = (L @ L.transpose(2, 3) / n + torch.eye(n, dtype=torch.float64)).float()
    c = rn(T, B, n).float()
    F = (0.1 * rn(T - 1, B, ns, n) + torch.cat((torch.eye(ns, dtype=torch.float64), torch.zeros(ns, nc, dtype=torch.float64)), 1)).float()
    f = (0.1 * rn(T - 1, B, ns)).float()
    return rn(B, ns).float(), C, c, F, f


def test_lqrstep_hands_the_family_code_only_under_the_flag():
    _native.load()
    x0, C, c, F, f = problem(13, 4)
    x = torch.zeros(4, 2, 13)
    u = torch.zeros(4, 2, 4)
    for flag, want in ((True, dict(kernel=_native.KKT_PREFER_NARROW)), (False, {}), (None, {})):
        be = SpyBackend()
        prev = _native.set_backend_for_testing(be)
        try:
            Cg = C.clone().requires_grad_(True)
            kw = {} if flag is None else dict(narrow_kkt_kernel=flag)
            step = LQRStep(13, 4, 4, current_x=x, current_u=u, no_op_forward=True, c_symmetric=True, **kw)
            nx, nu = step(x0, Cg, c, F, f)
            (nx.sum() + nu.sum()).backward()
        finally:
            _native.set_backend_for_testing(prev)
        assert be.backwards == [(13, 4, True, want)], (flag, be.backwards)
        assert Cg.grad is not None


def mpc_backward(be, ns, nc, flag, slew=True, T=4, B=2):
    x0, C, c, F, f = problem(ns, nc, T, B)
    prev = _native.set_backend_for_testing(be)
    try:
        Cg = C.clone().requires_grad_(True)
        kw = dict(slew_rate_penalty=1.0) if slew else {}
        kwf = dict(narrow_kkt_kernel=True) if flag else {}
        ctrl = mpc.MPC(ns, nc, T, u_lower=-1.0, u_upper=1.0, lqr_iter=3, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                       **kw, **kwf)
        x, u, _ = ctrl(x0, QuadCost(Cg, c), LinDx(F, f))
        (x.sum() + u.sum()).backward()
    finally:
        _native.set_backend_for_testing(prev)
    return Cg.grad


def test_mpc_makes_the_slew_endings_symmetry_promise_only_under_the_flag_and_only_where_the_loop_saw_a_symmetric_C():
    _native.load()
    narrow = dict(kernel=_native.KKT_PREFER_NARROW)
    on, off = SpyBackend(), SpyBackend()
    g_on, g_off = mpc_backward(on, 12, 4, True), mpc_backward(off, 12, 4, False)
    assert on.backwards == [(16, 4, True, narrow)]                   # the augmented problem, vouched for, the family asked for
    assert off.backwards == [(16, 4, False, {})]                     # as ever: no promise, no keyword
    assert torch.equal(g_on, g_off)                                  # (the stand-in solves both the same way)
    # the loop's first step reported a C that is not symmetric: no promise, the flag-off solve's gradients
    on, off = SpyBackend(asym=True), SpyBackend(asym=True)
    g_on, g_off = mpc_backward(on, 12, 4, True), mpc_backward(off, 12, 4, False)
    assert on.backwards == [(16, 4, False, narrow)] and off.backwards == [(16, 4, False, {})]
    assert torch.equal(g_on, g_off)
    # the plain ending: the promise is the one it always made, the flag adds the keyword
    on, off = SpyBackend(), SpyBackend()
    mpc_backward(on, 13, 4, True, slew=False), mpc_backward(off, 13, 4, False, slew=False)
    assert on.backwards == [(13, 4, True, narrow)] and off.backwards == [(13, 4, True, {})]
    assert mpc.MPC(13, 4, 4).narrow_kkt_kernel is False and mpc.MPC(13, 4, 4, narrow_kkt_kernel=True).narrow_step_kernel is False
