"""CPU-only: the closed-form part of the KKT backward with the kernel named by the caller (csrc/capi.hip: mpc_lqr_kkt_grads_kernel,
its two queries; csrc/kkt_wave64.hip; docs/history/r27.md) -- the declarations, MPC_KKT_GRADS_WAVE64, what the queries answer on
made-up pointers, and the flags `LQRStep(f64_grad_kernel=True)` / `mpc.MPC(f64_grad_kernel=True)` on a spying stand-in backend.

No call here reaches a launch; every pointer of the C calls is made up (the queries dereference none)."""
import ctypes
import importlib.util
import json
import os
import re

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
WAVE64 = 4
NAMES = ("mpc_lqr_kkt_grads_kernel_supported", "mpc_lqr_kkt_grads_kernel", "mpc_lqr_kkt_grads_kernel_route")
F64_SHAPES = [(1, 1), (12, 4), (13, 4), (32, 8), (60, 4), (63, 1)]


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def header():
    with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "mpc_lqr.h")) as fh:
        return fh.read()


def grads_pointers(T, ptr=gen.PTR):
    """dx, du, dl_dx, dl_du, dC, dc, dF, df, dx_init as tests/test_kkt_route_host.py makes them."""
    many = T > 1
    return (ptr,) * 6 + (ptr if many else None, ptr if many else None, ptr)


def test_the_header_declares_the_entries_and_the_binding_loads_them(lib):
    text = header()
    for name in NAMES:
        assert re.search(r"^int %s\(const mpc_lqr_problem \*p, int kernel[,)]" % name, text, re.M), name
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None


def test_the_code_is_four_here_and_there_and_the_abi_is_still_nine(lib):
    assert re.findall(r"^#define MPC_KKT_GRADS_WAVE64 (\d+)\b", header(), re.M) == ["4"]
    assert _native.KKT_GRADS_WAVE64 == WAVE64
    assert WAVE64 not in (_native.KKT_GRADS_DPP16, _native.KKT_GRADS_WAVE, _native.KKT_GRADS_GENERIC)
    assert int(lib.mpc_lqr_abi_version()) == 9 == _native.ABI_VERSION
    assert re.findall(r"^#define MPC_LQR_ABI_VERSION (\d+)", header(), re.M) == ["9"]


def test_build_info_names_the_kernels(lib):
    assert "kkt_grads_wave<f64>" in lib.mpc_lqr_build_info().decode()


def test_supported_looks_at_sizes_and_dtype(lib):
    for ns, nc in F64_SHAPES:
        for T, B in ((1, 1), (5, 3), (50, 1024), (4, 0)):
            p = gen.problem(_native, ns, nc, _native.MPC_F64, T, B)
            assert int(lib.mpc_lqr_kkt_grads_kernel_supported(r(p), WAVE64)) == 1, (ns, nc, T, B)
        p32 = gen.problem(_native, ns, nc, _native.MPC_F32, 5, 3)
        assert int(lib.mpc_lqr_kkt_grads_kernel_supported(r(p32), WAVE64)) == 0, (ns, nc)
        for code in (0, 1, 2, 3, 99):
            assert int(lib.mpc_lqr_kkt_grads_kernel_supported(r(p), code)) == 0, (ns, nc, code)
    for ns, nc in ((61, 4), (64, 1)):
        p = gen.problem(_native, ns, nc, _native.MPC_F64, 5, 3)
        assert int(lib.mpc_lqr_kkt_grads_kernel_supported(r(p), WAVE64)) == 0, (ns, nc)
    # pointers play no part: a problem with none
    bare = _native.Problem()
    bare.B, bare.T, bare.ns, bare.nc, bare.dtype = 3, 5, 12, 4, _native.MPC_F64
    assert int(lib.mpc_lqr_kkt_grads_kernel_supported(r(bare), WAVE64)) == 1
    assert int(lib.mpc_lqr_kkt_grads_kernel_supported(None, WAVE64)) == 0


def test_the_route_answers_four_where_the_kernel_takes_the_call(lib):
    for ns, nc in F64_SHAPES:
        for T in (1, 5):
            p = gen.problem(_native, ns, nc, _native.MPC_F64, T, 3)
            if T == 1:
                p.F = None
            assert int(lib.mpc_lqr_kkt_grads_kernel_route(r(p), WAVE64, *grads_pointers(T))) == WAVE64, (ns, nc, T, lib.mpc_lqr_last_error())
            # ... on 8 bytes but not 16, and on strides that are odd: the general form, the same code
            p = gen.problem(_native, ns, nc, _native.MPC_F64, T, 3, ptr=gen.PTR + 8, skew=1)
            if T == 1:
                p.F = None
            assert int(lib.mpc_lqr_kkt_grads_kernel_route(r(p), WAVE64, *grads_pointers(T, gen.PTR + 8))) == WAVE64, (ns, nc, T)
    p = gen.problem(_native, 12, 4, _native.MPC_F64, 5, 0)
    assert int(lib.mpc_lqr_kkt_grads_kernel_route(r(p), WAVE64, *grads_pointers(5))) == 0           # B = 0: nothing would launch
    assert int(lib.mpc_lqr_kkt_grads_kernel(r(p), WAVE64, *grads_pointers(5), None)) == 0           # ... and nothing does


def test_the_route_refuses_with_the_entrys_code_and_text(lib):
    p = gen.problem(_native, 12, 4, _native.MPC_F64, 5, 3)
    ptrs = grads_pointers(5)
    for entry in (lambda *a: lib.mpc_lqr_kkt_grads_kernel_route(*a), lambda *a: lib.mpc_lqr_kkt_grads_kernel(*a, None)):
        # the shared checks of mpc_lqr_kkt_grads, with its texts
        for i, text in ((0, "kkt_grads: NULL argument"), (5, "kkt_grads: NULL argument"), (6, "kkt_grads: dF is NULL")):
            args = ptrs[:i] + (None,) + ptrs[i + 1:]
            assert int(entry(r(p), WAVE64, *args)) == E_NULL and lib.mpc_lqr_last_error().decode() == text
            assert int(lib.mpc_lqr_kkt_grads_route(r(p), *args)) == E_NULL and lib.mpc_lqr_last_error().decode() == text
        # the kernel's own: float64, its sizes, 8-byte pointers -- each names the kernel
        p32 = gen.problem(_native, 12, 4, _native.MPC_F32, 5, 3)
        assert int(entry(r(p32), WAVE64, *ptrs)) == E_DIMS
        text = lib.mpc_lqr_last_error().decode()
        assert "MPC_KKT_GRADS_WAVE64" in text and "float64" in text, text
        for ns, nc in ((61, 4), (64, 1)):
            big = gen.problem(_native, ns, nc, _native.MPC_F64, 5, 3)
            assert int(entry(r(big), WAVE64, *ptrs)) == E_DIMS
            text = lib.mpc_lqr_last_error().decode()
            assert "MPC_KKT_GRADS_WAVE64" in text and "2 <= n_state + n_ctrl <= 64" in text, text
        off = ptrs[:4] + (gen.PTR + 4,) + ptrs[5:]
        assert int(entry(r(p), WAVE64, *off)) == E_DIMS
        text = lib.mpc_lqr_last_error().decode()
        assert "MPC_KKT_GRADS_WAVE64" in text and "8-byte" in text, text
        # float32 at a size beyond the kernel: the dtype is the first thing it misses
        assert int(entry(r(gen.problem(_native, 64, 1, _native.MPC_F32, 5, 3)), WAVE64, *ptrs)) == E_DIMS
        assert "float64" in lib.mpc_lqr_last_error().decode()
        for code in (1, 2, 3, 5, 99, -1):
            assert int(entry(r(p), code, *ptrs)) == E_ARG, code
            assert "unknown kernel code" in lib.mpc_lqr_last_error().decode()


def test_kernel_zero_is_the_existing_query_row_by_row(lib):
    with open(os.path.join(GOLDEN, "kkt_route_expect.json")) as fh:
        t = json.load(fh)
    rows = [dict(t["defaults"], **row) for row in t["rows"]]
    assert {row["dtype"] for row in rows} >= {"f32", "f64"}
    for row in rows:
        ns, nc = row["shape"]
        T, B = row["T"], row["B"]
        at = lambda name: gen.PTR + row["off"].get(name, 0)
        p = gen.problem(_native, ns, nc, _native.MPC_F32 if row["dtype"] == "f32" else _native.MPC_F64, T, B)
        for name in ("x_init", "C", "c", "F", "f", "cur_x", "cur_u"):
            setattr(p, name, at(name))
        for name, more in row["skew"].items():
            setattr(p, name, getattr(p, name) + more)
        for name, value in row["set"].items():
            setattr(p, name, value)
        if T == 1:
            p.F = None
        many = T > 1
        grads = (at("dx"), at("du"), at("dl_dx"), at("dl_du"), at("dC"), at("dc"), at("dF") if many else None, at("df") if many else None,
                 at("dx_init"))
        want = int(lib.mpc_lqr_kkt_grads_route(r(p), *grads))
        assert want == getattr(_native, "KKT_GRADS_" + row["grads"]), row["id"]
        assert int(lib.mpc_lqr_kkt_grads_kernel_route(r(p), 0, *grads)) == want, row["id"]
    # ... and its refusals
    p = gen.problem(_native, 12, 4, _native.MPC_F64, 5, 3)
    args = (None,) + grads_pointers(5)[1:]
    assert int(lib.mpc_lqr_kkt_grads_kernel_route(r(p), 0, *args)) == E_NULL == int(lib.mpc_lqr_kkt_grads_kernel(r(p), 0, *args, None))
    assert lib.mpc_lqr_last_error().decode() == "kkt_grads: NULL argument"


# ---------------------------------------------------------------------------------------------
# the flags, on a stand-in backend that records what the backward is handed
# ---------------------------------------------------------------------------------------------
class SpyBackend(OracleBackend):
    def __init__(self):
        super().__init__()
        self.backwards = []

    def kkt_backward(self, C, c, F, f, x_star, u_star, dl_dx, dl_du, opts, impl=0, **kw):
        self.backwards.append((x_star.shape[2], u_star.shape[2], C.dtype, dict(kw)))
        return super().kkt_backward(C, c, F, f, x_star, u_star, dl_dx, dl_du, opts, impl=impl)


def problem(ns, nc, T=4, B=2):
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    n = ns + nc
    L = rn(T, B, n, n)
    C = L @ L.transpose(2, 3) / n + torch.eye(n, dtype=torch.float64)
    F = 0.1 * rn(T - 1, B, ns, n) + torch.cat((torch.eye(ns, dtype=torch.float64), torch.zeros(ns, nc, dtype=torch.float64)), 1)
    return rn(B, ns), C, rn(T, B, n), F, 0.1 * rn(T - 1, B, ns)


def test_lqrstep_hands_the_code_only_under_the_flag():
    _native.load()
    x0, C, c, F, f = problem(12, 4)
    x, u = torch.zeros(4, 2, 12, dtype=torch.float64), torch.zeros(4, 2, 4, dtype=torch.float64)
    for flag, want in ((True, dict(grads_kernel=_native.KKT_GRADS_WAVE64)), (False, {}), (None, {})):
        be = SpyBackend()
        prev = _native.set_backend_for_testing(be)
        try:
            Cg = C.clone().requires_grad_(True)
            kw = {} if flag is None else dict(f64_grad_kernel=flag)
            step = LQRStep(12, 4, 4, current_x=x, current_u=u, no_op_forward=True, **kw)
            nx, nu = step(x0, Cg, c, F, f)
            (nx.sum() + nu.sum()).backward()
        finally:
            _native.set_backend_for_testing(prev)
        assert be.backwards == [(12, 4, torch.float64, want)], (flag, be.backwards)
        assert Cg.grad is not None


def test_the_batch_shared_backward_hands_the_code_to_its_kkt_backward_fallback():
    _native.load()
    x0, C, c, F, f = problem(12, 4)
    x, u = torch.zeros(4, 2, 12, dtype=torch.float64), torch.zeros(4, 2, 4, dtype=torch.float64)
    for flag, want in ((True, dict(grads_kernel=_native.KKT_GRADS_WAVE64)), (False, {})):
        be = SpyBackend()
        assert not hasattr(be, "kkt_backward_shared")
        prev = _native.set_backend_for_testing(be)
        try:
            Cs = C[:, 0].clone().requires_grad_(True)                       # batch-shared: [T,n,n]
            step = LQRStep(12, 4, 4, current_x=x, current_u=u, no_op_forward=True, shared_grad_kernel=True, f64_grad_kernel=flag)
            nx, nu = step(x0, Cs, c, F, f)
            (nx.sum() + nu.sum()).backward()
        finally:
            _native.set_backend_for_testing(prev)
        assert be.backwards == [(12, 4, torch.float64, want)], (flag, be.backwards)
        assert Cs.grad is not None and Cs.grad.shape == Cs.shape


def mpc_backward(be, ns, nc, flag, slew, T=4, B=2):
    x0, C, c, F, f = problem(ns, nc, T, B)
    prev = _native.set_backend_for_testing(be)
    try:
        Cg = C.clone().requires_grad_(True)
        kw = dict(slew_rate_penalty=1.0) if slew else {}
        kwf = dict(f64_grad_kernel=True) if flag else {}
        ctrl = mpc.MPC(ns, nc, T, u_lower=-1.0, u_upper=1.0, lqr_iter=3, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                       **kw, **kwf)
        x, u, _ = ctrl(x0, QuadCost(Cg, c), LinDx(F, f))
        (x.sum() + u.sum()).backward()
    finally:
        _native.set_backend_for_testing(prev)
    return Cg.grad


def test_mpc_reaches_the_final_step_with_the_flag_on_both_endings():
    _native.load()
    code = dict(grads_kernel=_native.KKT_GRADS_WAVE64)
    for slew, sizes in ((False, (12, 4)), (True, (16, 4))):              # (the slew ending differentiates the augmented problem)
        on, off = SpyBackend(), SpyBackend()
        g_on, g_off = mpc_backward(on, 12, 4, True, slew), mpc_backward(off, 12, 4, False, slew)
        assert on.backwards == [sizes + (torch.float64, code)], (slew, on.backwards)
        assert off.backwards == [sizes + (torch.float64, {})], (slew, off.backwards)
        assert torch.equal(g_on, g_off)                                  # (the stand-in solves both the same way)
    assert mpc.MPC(12, 4, 4).f64_grad_kernel is False and mpc.MPC(12, 4, 4, f64_grad_kernel=True).f64_grad_kernel is True
    import inspect
    assert inspect.signature(mpc.MPC.__init__).parameters["f64_grad_kernel"].default is False
    assert inspect.signature(LQRStep).parameters["f64_grad_kernel"].default is False
