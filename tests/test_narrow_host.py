"""CPU-only: impl 9 (MPC_IMPL_MFMA40_NARROW, the padded 32/8 kernel on one 16-row state tile) in the host-side decisions -- the
envelope of mpc_lqr_impl_supported, mpc_lqr_step_route for a forced 9, what impl 0 keeps answering, the workspace size and the
qp record -- and `MPC(narrow_step_kernel=True)` on a spying stand-in backend.  No call here reaches a launch; every pointer of
the C calls is made up (the queries dereference none)."""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN
from mpc import _native, mpc
from mpc.mpc import LinDx, QuadCost
from oracle_backend import OracleBackend

_spec = importlib.util.spec_from_file_location("make_golden_step_route", os.path.join(GOLDEN, "make_golden_step_route.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
NARROW, PAD = 9, 7
r = ctypes.byref


@pytest.fixture
def lib(monkeypatch):
    monkeypatch.delenv("MPC_DPP16_RING", raising=False)
    monkeypatch.delenv("MPC_MFMA40_RING", raising=False)
    _native.load()
    L = gen.bind(_native)
    L.mpc_lqr_step_route.argtypes = L.mpc_lqr_step.argtypes[:6] + [ctypes.POINTER(ctypes.c_int)]
    return L


def test_the_python_constant_is_the_c_one():
    assert _native.IMPL_MFMA40_NARROW == NARROW and _native.IMPL_MFMA40_PAD == PAD


def supported(L, ns, nc, dtype=None, o=None, impl=NARROW):
    p = gen.problem(_native, ns, nc, _native.MPC_F32 if dtype is None else dtype, 5, 3)
    return int(L.mpc_lqr_impl_supported(r(p), None if o is None else r(o), impl))


def test_impl_supported_over_the_envelope_and_just_outside(lib):
    for ns, nc in ((1, 1), (5, 3), (12, 4), (13, 4), (16, 4), (16, 8), (9, 6), (1, 8), (16, 1)):
        assert supported(lib, ns, nc) == 1, (ns, nc)
        assert supported(lib, ns, nc, o=gen.options(_native, box=1)[0]) == 1
        assert supported(lib, ns, nc, o=gen.options(_native, box=2)[0]) == 1
        assert supported(lib, ns, nc, o=gen.options(_native, max_ls=16)[0]) == 1
    for ns, nc in ((17, 4), (17, 8), (16, 9), (32, 8), (20, 5), (0, 4), (16, 0)):
        assert supported(lib, ns, nc) == 0, (ns, nc)
    assert supported(lib, 17, 4, impl=PAD) == 1                      # (the padded kernel's envelope is where it was)
    assert supported(lib, 16, 4, dtype=_native.MPC_F64) == 0
    assert supported(lib, 16, 4, o=gen.options(_native, max_ls=17)[0]) == 0
    o, _ = gen.options(_native, box=1)
    o.zero_mask = gen.PTR
    assert supported(lib, 16, 4, o=o) == 0                           # box together with u_zero_I, as impl 7
    o, _ = gen.options(_native)
    o.zero_mask = gen.PTR
    assert supported(lib, 16, 4, o=o) == 1
    o, _e = gen.options(_native, env=(1, 0))
    assert supported(lib, 3, 1, o=o) == 0                            # a simulator
    assert supported(lib, 16, 4, impl=10) == 0


def route(L, ns, nc, impl, dtype=None, o=None, ws="full", gains=True, T=5, B=3):
    p = gen.problem(_native, ns, nc, _native.MPC_F32 if dtype is None else dtype, T, B)
    if o is None:
        o = gen.options(_native)[0]
    out = gen.outputs(_native, gains=gains)
    full = int(L.mpc_lqr_workspace_bytes(r(p)))
    w, nbytes = {"full": (gen.WS, full), "misaligned": (gen.WS + 4, full), "none": (None, 0), "small": (gen.WS, full // 8)}[ws]
    ring = ctypes.c_int(-1)
    rc = int(L.mpc_lqr_step_route(r(p), r(o), r(out), w, nbytes, impl, r(ring)))
    return rc, L.mpc_lqr_last_error().decode(), ring.value


def test_a_forced_9_is_answered_9_or_refused_with_the_steps_code_and_text(lib):
    for ns, nc in ((13, 4), (16, 4), (16, 8), (9, 6), (5, 3), (12, 4), (1, 1)):
        for box in (0, 1, 2):
            for gains in (True, False):
                rc, _, ring = route(lib, ns, nc, NARROW, o=gen.options(_native, box=box)[0], gains=gains)
                assert (rc, ring) == (NARROW, 0), (ns, nc, box, gains)
        assert route(lib, ns, nc, NARROW, o=gen.options(_native, flags=gen.OPT_SWEEP_ONLY)[0])[0] == NARROW
    text = "narrow MFMA kernel needs fp32, n_state <= 16, n_ctrl <= 8, max_linesearch_iter <= 16, no simulator, and the " \
           "workspace of mpc_lqr_workspace_bytes (16-byte aligned)"
    E_DIMS = route(lib, 33, 8, PAD)[0]
    assert E_DIMS < 0
    for kw in (dict(ns=17, nc=4), dict(ns=16, nc=9), dict(ns=20, nc=5), dict(ns=16, nc=4, ws="none"), dict(ns=16, nc=4, ws="misaligned"),
               dict(ns=16, nc=4, ws="small", T=50, B=64), dict(ns=16, nc=4, o=gen.options(_native, max_ls=17)[0])):
        rc, msg, _ = route(lib, kw.pop("ns"), kw.pop("nc"), NARROW, **kw)
        assert (rc, msg) == (E_DIMS, text), kw
    o, _ = gen.options(_native, box=1)
    o.zero_mask = gen.PTR
    assert route(lib, 16, 4, NARROW, o=o)[:2] == (E_DIMS, text)
    rc, msg, _ = route(lib, 16, 4, NARROW, dtype=_native.MPC_F64)
    assert rc < 0 and rc != E_DIMS and msg == "the narrow MFMA kernel is fp32 only"
    # the padded kernel refuses its own way, as before
    assert route(lib, 33, 8, PAD)[1].startswith("padded MFMA kernel needs fp32, n_state <= 32")


def expected_routes():
    with open(os.path.join(GOLDEN, "step_route_expect.json")) as fh:
        t = json.load(fh)
    return [dict(t["defaults"], **row) for row in t["rows"]]


def test_auto_never_answers_9(lib):
    """every row of the hand-written route table under impl 0 (and under the impl it names) keeps its kernel"""
    for row in expected_routes():
        ns, nc = row["shape"]
        dtype = _native.MPC_F32 if row["dtype"] == "f32" else _native.MPC_F64
        p = gen.problem(_native, ns, nc, dtype, row["T"], row["B"], ptr=gen.PTR + (0 if row["align"] == 16 else 4))
        o, _keep = gen.options(_native, box={"none": 0, "scalar": 1, "tensor": 2}[row["bounds"]], max_ls=row["max_ls"],
                               flags=gen.OPT_SWEEP_ONLY if row["sweep_only"] else 0)
        if row["mask"]:
            o.zero_mask = gen.PTR
        out = gen.outputs(_native, gains=row["gains"])
        full = int(lib.mpc_lqr_workspace_bytes(r(p)))
        ws, nbytes = {"full": (gen.WS, full), "misaligned": (gen.WS + 4, full), "none": (None, 0)}[row["workspace"]]
        for impl in {0, row["impl"]}:
            k = int(lib.mpc_lqr_step_route(r(p), r(o), r(out), ws, nbytes, impl, None))
            assert k != NARROW and (impl != row["impl"] or k == row["kernel"]), (row["id"], impl, k)


def test_workspace_bytes_are_the_recorded_ones(lib):
    with open(os.path.join(GOLDEN, "step_route_answers.json")) as fh:
        table = gen.unpack(json.load(fh))
    for want in table:
        got = [int(lib.mpc_lqr_workspace_bytes(r(gen.problem(_native, want["n_state"], want["n_ctrl"], want["dtype"], T, B)))) for T, B in gen.SIZES]
        assert got == want["workspace_bytes"], (want["n_state"], want["n_ctrl"], want["dtype"])


def test_qp_record_for_9_is_the_answer_for_7(lib):
    for ns, nc in ((13, 4), (16, 4), (16, 8), (5, 3), (12, 4)):
        for align, kw in (("aligned", {}), ("pointers+4", dict(ptr=gen.PTR + 4)), ("strides+1", dict(skew=1))):
            p = gen.problem(_native, ns, nc, _native.MPC_F32, 5, 3, **kw)
            for box in (0, 1, 2):
                o, _ = gen.options(_native, box=box)
                cells = []
                for impl in (PAD, NARROW):
                    off, st, sb = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
                    cells.append([int(lib.mpc_lqr_qp_record(r(p), r(o), impl, r(off), r(st), r(sb))), off.value, st.value, sb.value])
                assert cells[0] == cells[1], (ns, nc, align, box, cells)
                assert cells[0][0] == (1 if box else 0)
    # ... and none where the narrow kernel does not take the step
    p = gen.problem(_native, 20, 5, _native.MPC_F32, 5, 3)
    off = ctypes.c_int64(-7)
    assert int(lib.mpc_lqr_qp_record(r(p), r(gen.options(_native, box=1)[0]), NARROW, r(off), r(off), r(off))) == 0


# ---------------------------------------------------------------------------------------------
# MPC(narrow_step_kernel=...) on a stand-in backend that records the impl of every plan
# ---------------------------------------------------------------------------------------------
class SpyBackend(OracleBackend):
    """asym: a step / sweep FORCED onto impl 9 reports MPC_ST_C_ASYMMETRIC (8) on problem 0, as the kernel does for a C that is
    not symmetric (impl 0 re-solves such a problem inside the call: the stand-in's auto plans report nothing)"""

    def __init__(self, says=None, asym=False):
        super().__init__()
        self.says, self.asym, self.asked, self.plans, self.net_plans = says, asym, [], [], []

    def impl_supported(self, ns, nc, dtype, impl, opts=None):
        self.asked.append((ns, nc, impl))
        if self.says is not None and impl == NARROW:
            return self.says
        return _native.HipBackend.impl_supported(None, ns, nc, dtype, impl, opts)       # the library's own answer (a host call)

    def _flag(self, r, impl):
        if self.asym and impl == NARROW:
            r["status"] = r["status"].clone()
            r["status"][0] |= 8
        return r

    def plan_step(self, x_init, C, c, F, f, cur_x, cur_u, opts, impl=0, **kw):
        self.plans.append((x_init.shape[1], C.shape[2] - x_init.shape[1], impl))
        run = super().plan_step(x_init, C, c, F, f, cur_x, cur_u, opts, impl=impl, **kw)
        return lambda: self._flag(run(), impl)

    def plan_network_iteration(self, x_init, C, c, net, opts, nominals, scratch=None, impl=0):
        self.net_plans.append((x_init.shape[1], C.shape[2] - x_init.shape[1], impl))
        run, outs, vouch = super().plan_network_iteration(x_init, C, c, net, opts, nominals, scratch)
        return (lambda j, stream=None: self._flag(run(j, stream), impl)), outs, vouch


def solve(be, ns, nc, flag=True, slew=False, T=4, B=2):
    prev = _native.set_backend_for_testing(be)
    try:
        g = torch.Generator().manual_seed(3)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        n = ns + nc
        L = rn(T, B, n, n)
        C = (L @ L.transpose(2, 3) / n + torch.eye(n, dtype=torch.float64)).float()
        c = rn(T, B, n).float()
        F = (0.1 * rn(T - 1, B, ns, n) + torch.cat((torch.eye(ns, dtype=torch.float64), torch.zeros(ns, nc, dtype=torch.float64)), 1)).float()
        f = (0.1 * rn(T - 1, B, ns)).float()
        x0 = rn(B, ns).float()
        kw = dict(slew_rate_penalty=1.0) if slew else {}
        kwf = dict(narrow_step_kernel=True) if flag else {}
        ctrl = mpc.MPC(ns, nc, T, u_lower=-1.0, u_upper=1.0, lqr_iter=3, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                       backprop=False, **kw, **kwf)
        with torch.no_grad():
            be.result = ctrl(x0, QuadCost(C, c), LinDx(F, f))
    finally:
        _native.set_backend_for_testing(prev)
    return be.plans


def test_the_flag_binds_impl_9_where_the_backend_takes_the_sizes():
    _native.load()
    plans = solve(SpyBackend(), 13, 4)
    assert plans and all(pl == (13, 4, NARROW) for pl in plans), plans
    plans = solve(SpyBackend(), 12, 4, slew=True)                    # the augmentation: 16/4
    assert plans and all(pl == (16, 4, NARROW) for pl in plans), plans
    plans = solve(SpyBackend(), 9, 6)
    assert plans and all(pl == (9, 6, NARROW) for pl in plans), plans


def test_the_flag_keeps_impl_0_everywhere_else():
    _native.load()
    plans = solve(SpyBackend(), 12, 4)                               # 12/4 without a penalty: its own kernels, auto's choice
    assert plans and all(pl == (12, 4, 0) for pl in plans), plans
    plans = solve(SpyBackend(), 20, 5)
    assert plans and all(pl == (20, 5, 0) for pl in plans), plans
    be = SpyBackend(says=False)
    plans = solve(be, 13, 4)
    assert plans and all(pl == (13, 4, 0) for pl in plans) and (13, 4, NARROW) in be.asked
    be = SpyBackend()
    plans = solve(be, 13, 4, flag=False)
    assert plans and all(pl == (13, 4, 0) for pl in plans) and not be.asked
    plans = solve(SpyBackend(), 12, 4, flag=False, slew=True)
    assert plans and all(pl == (16, 4, 0) for pl in plans), plans
    assert mpc.MPC(13, 4, 4).narrow_step_kernel is False


def test_a_nonsymmetric_C_reported_by_the_forced_kernel_starts_the_loop_over_on_auto():
    """A forced kernel only flags a C that is not symmetric (impl 0 repairs it inside the call): the narrow-bound loop binds its
    plans again with IMPL_AUTO, runs iteration 0 again from the same nominal and is the flag-off solve from there on."""
    _native.load()
    for ns, nc, slew, at in ((13, 4, False, (13, 4)), (12, 4, True, (16, 4))):
        on, off = SpyBackend(asym=True), SpyBackend(asym=True)
        plans = solve(on, ns, nc, slew=slew)
        assert plans == [at + (NARROW,)] * 2 + [at + (0,)] * 2, plans        # no c_symmetric plans: C is not symmetric
        assert solve(off, ns, nc, flag=False, slew=slew) == [at + (0,)] * 4
        steps = lambda be: [k for k in be.calls if k.startswith("step:")]
        assert len(steps(on)) == len(steps(off)) + 1 and steps(on)[:2] == ["step:c_unknown"] * 2
        for a, b in zip(on.result, off.result):
            assert torch.equal(a, b)
        # ... and a symmetric C costs nothing but the held-back second launch: the same steps as with the flag off
        on, off = SpyBackend(), SpyBackend()
        solve(on, ns, nc, slew=slew), solve(off, ns, nc, flag=False, slew=slew)
        assert steps(on) == steps(off)
        for a, b in zip(on.result, off.result):
            assert torch.equal(a, b)


def net_solve(be, flag, monkeypatch, ns=13, nc=4, T=5, B=3):
    from mpc.dynamics import NNDynamics
    monkeypatch.setattr(_native.MlpSpec, "supported", staticmethod(lambda weights, activation, like, bits=3: True))
    torch.manual_seed(3)
    dyn = NNDynamics(ns, nc, [12], activation="sigmoid")
    A = torch.randn(T, B, ns + nc, ns + nc)
    C = A.transpose(2, 3).matmul(A) + 0.1 * torch.eye(ns + nc)
    c = torch.randn(T, B, ns + nc)
    x0 = torch.randn(B, ns)
    u0 = 0.2 * torch.randn(T, B, nc)
    prev = _native.set_backend_for_testing(be)
    try:
        ctrl = mpc.MPC(ns, nc, T, u_lower=-0.5, u_upper=0.5, lqr_iter=4, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                       grad_method=mpc.GradMethods.ANALYTIC, backprop=False, u_init=u0.clone(), narrow_step_kernel=flag)
        with torch.no_grad():
            return ctrl(x0, QuadCost(C, c), dyn)
    finally:
        _native.set_backend_for_testing(prev)


def test_the_network_loop_binds_its_sweep_with_impl_9_and_starts_over_on_a_nonsymmetric_C(monkeypatch):
    _native.load()
    iters = lambda be: [k for k in be.calls if k.startswith("network_iteration")]
    on, off = SpyBackend(), SpyBackend()
    r_on, r_off = net_solve(on, True, monkeypatch), net_solve(off, False, monkeypatch)
    assert on.net_plans == [(13, 4, NARROW)] and off.net_plans == [(13, 4, 0)] and not on.plans
    assert iters(on) == iters(off) and "network_iteration:c_symmetric" in iters(on)
    for a, b in zip(r_on, r_off):
        assert torch.equal(a, b)
    on, off = SpyBackend(asym=True), SpyBackend(asym=True)
    r_on, r_off = net_solve(on, True, monkeypatch), net_solve(off, False, monkeypatch)
    assert on.net_plans == [(13, 4, NARROW), (13, 4, 0)] and off.net_plans == [(13, 4, 0)]
    assert len(iters(on)) == len(iters(off)) + 1
    for a, b in zip(r_on, r_off):
        assert torch.equal(a, b)
    assert net_solve(SpyBackend(), True, monkeypatch, ns=4, nc=2) is not None            # 4/2: the 12/4-class kernels' shape
