"""CPU tests of the batch-summed KKT gradients (csrc/kkt_shared.hip, mpc_lqr_kkt_grads_shared, HipBackend.kkt_backward_shared,
lqr_step._LQRStepSharedFn, `shared_grad_kernel=`): the routing of LQRStep and mpc.MPC on a spying oracle backend in float64,
`want` against needs_input_grad, LinDx in 2- and 3-dimensional form, and the C entry's argument checks (no device needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from mpc import _native, lqr_step as LS, mpc, util
from mpc.lqr_step import LQRStep
from mpc.mpc import LinDx, QuadCost
from oracle import lqr_oracle as O
from oracle_backend import OracleBackend, _bound, _np

T, B, NS, NC = 5, 4, 3, 2
N = NS + NC
NAMES = ("C", "c", "F", "f")


class SharedOracleBackend(OracleBackend):
    """The stand-in with `kkt_backward_shared`: the oracle's per-problem gradients added over the batch in float64."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.wants = []
        self.returned = []

    def kkt_backward_shared(self, C, c, F, f, x_star, u_star, dl_dx, dl_du, opts, want=(True, True, True, True)):
        self.calls.append("kkt_backward_shared")
        self.wants.append(tuple(want))
        o = O.kkt_backward(_np(C), _np(c), _np(F), _np(f), _np(x_star), _np(u_star), _np(dl_dx.to(C.dtype)), _np(dl_du.to(C.dtype)),
                           _bound(opts.u_lower), _bound(opts.u_upper), lockstep=self.lockstep)
        out = {k: self._t(o[k], C) for k in ("dx_init", "dx", "du")}
        for name, src, w in zip(("sum_dC", "sum_dc", "sum_dF", "sum_df"), ("dC", "dc", "dF", "df"), want):
            out[name] = self._t(o[src].sum(1), C) if (w and o[src] is not None) else None
        self.returned.append({k: (None if v is None else tuple(v.shape)) for k, v in out.items()})
        return out


@pytest.fixture
def use():
    installed = []

    def install(be):
        installed.append(_native.set_backend_for_testing(be))
        return be
    yield install
    for prev in reversed(installed):
        _native.set_backend_for_testing(prev)


def bases(time_invariant=False, seed=0):
    """A convex shared problem in float64: C, c, F, f in base form ([T,...], or without the T axis), x_init [B,ns] and the
    weights of a linear loss on (x, u)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    lead_c, lead_f = ((), ()) if time_invariant else ((T,), (T - 1,))
    L = r(*lead_c, N, N)
    C = L.transpose(-1, -2) @ L + torch.eye(N, dtype=torch.float64)
    c = r(*lead_c, N)
    F = torch.cat((torch.eye(NS, dtype=torch.float64).expand(*lead_f, NS, NS) + 0.2 * r(*lead_f, NS, NS), r(*lead_f, NS, NC)), -1)
    f = 0.3 * r(*lead_f, NS)
    return dict(C=C, c=c, F=F, f=f, x_init=r(B, NS), wx=r(T, B, NS), wu=r(T, B, NC))


def views(leaves):
    """The caller-made [T,B,...] `.expand()` views of base-form leaves."""
    return [LS._expand_shared(leaves[k], i, T, B) for i, k in enumerate(NAMES)]


def leaves_of(p, full=(), no_grad=()):
    """Fresh leaves of the problem's C, c, F, f; the names in `full` as contiguous full-rank [T,B,...] leaves."""
    out = {}
    for i, k in enumerate(NAMES):
        t = p[k].clone()
        if k in full:
            t = LS._expand_shared(t, i, T, B).contiguous()
        out[k] = t.requires_grad_(k not in no_grad)
    return out


def nominal(p):
    u = torch.zeros(T, B, NC, dtype=torch.float64)
    Fv, fv = views(p)[2:]
    return util.get_traj(T, u, x_init=p["x_init"], dynamics=LinDx(Fv, fv)), u


def step_grads(p, leaves, args, no_op, **kw):
    """d loss / d leaves of one LQRStep on `args` (C, c, F, f as the step is to see them)."""
    x, u = nominal(p)
    if no_op:                                        # attach the backward at the step's own solution
        with torch.no_grad():
            x, u = LQRStep(NS, NC, T, u_lower=-0.4, u_upper=0.4, current_x=x, current_u=u)(p["x_init"], *views(p))[:2]
    out = LQRStep(NS, NC, T, u_lower=-0.4, u_upper=0.4, current_x=x, current_u=u, no_op_forward=no_op, **kw)(p["x_init"], *args)
    loss = (out[0] * p["wx"]).sum() + (out[1] * p["wu"]).sum()
    return torch.autograd.grad(loss, [leaves[k] for k in NAMES if leaves[k].requires_grad])


def assert_close(got, ref):
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max()))


def spy_backward(monkeypatch):
    seen = []
    orig = LS._LQRStepSharedFn.backward

    def spy(ctx, *grads):
        out = orig(ctx, *grads)
        seen.append([None if v is None else tuple(v.shape) for v in out])
        return out
    monkeypatch.setattr(LS._LQRStepSharedFn, "backward", staticmethod(spy))
    return seen


# ---------------------------------------------------------------------------------------------
# 1. routing: LQRStep
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_op", (False, True))
@pytest.mark.parametrize("time_invariant", (False, True))
def test_lqrstep_takes_the_summed_route_for_shared_arguments(use, monkeypatch, no_op, time_invariant):
    p = bases(time_invariant)
    seen = spy_backward(monkeypatch)
    be = use(SharedOracleBackend())
    lv = leaves_of(p)
    got = step_grads(p, lv, [lv[k] for k in NAMES], no_op, shared_grad_kernel=True)
    assert be.calls.count("kkt_backward_shared") == 1 and "kkt_backward" not in be.calls
    assert be.wants == [(True, True, True, True)]
    # what the backend handed over, and what the Function handed to autograd: nothing with a batch axis but dx_init
    assert be.returned[0]["sum_dC"] == (T, N, N) and be.returned[0]["sum_dF"] == (T - 1, NS, N)
    assert seen == [[None, (B, NS)] + [tuple(p[k].shape) for k in NAMES]]
    # the parent's route on the same problem: caller-made views, per-problem gradients, autograd's sum through the expand
    ref_be = use(OracleBackend())
    lr = leaves_of(p)
    ref = step_grads(p, lr, views(lr), no_op)
    assert "kkt_backward" in ref_be.calls
    assert_close(got, ref)
    assert all(g.shape == p[k].shape for g, k in zip(got, NAMES))


def test_lqrstep_declines_when_a_full_rank_argument_needs_a_gradient(use, monkeypatch):
    p = bases()
    seen = spy_backward(monkeypatch)
    be = use(SharedOracleBackend())
    lv = leaves_of(p, full=("C",))
    got = step_grads(p, lv, [lv[k] for k in NAMES], True, shared_grad_kernel=True)
    assert "kkt_backward_shared" not in be.calls and be.calls.count("kkt_backward") == 1
    assert seen[0][2] == (T, B, N, N) and seen[0][3:] == [tuple(p[k].shape) for k in NAMES[1:]]
    use(OracleBackend())
    lr = leaves_of(p, full=("C",))
    assert_close(got, step_grads(p, lr, views(lr), True))


def test_lqrstep_full_rank_argument_without_gradient_does_not_decline(use):
    p = bases()
    be = use(SharedOracleBackend())
    lv = leaves_of(p, full=("F",), no_grad=("F",))
    got = step_grads(p, lv, [lv[k] for k in NAMES], True, shared_grad_kernel=True)
    assert be.calls.count("kkt_backward_shared") == 1 and be.wants == [(True, True, False, True)]
    use(OracleBackend())
    lr = leaves_of(p, full=("F",), no_grad=("F",))
    assert_close(got, step_grads(p, lr, views(lr), True))


def test_lqrstep_declines_reference_du_norm_and_backends_without_the_method(use):
    p = bases()
    lr = leaves_of(p)
    use(OracleBackend())
    ref = step_grads(p, lr, views(lr), False)
    be = use(SharedOracleBackend())
    lv = leaves_of(p)
    got = step_grads(p, lv, [lv[k] for k in NAMES], False, shared_grad_kernel=True, reference_du_norm=True)
    assert "kkt_backward_shared" not in be.calls and "kkt_backward" in be.calls
    assert_close(got, ref)
    plain = use(OracleBackend())
    assert not hasattr(plain, "kkt_backward_shared")
    lv = leaves_of(p)
    got = step_grads(p, lv, [lv[k] for k in NAMES], False, shared_grad_kernel=True)
    assert plain.calls.count("kkt_backward") == 1
    assert_close(got, ref)


# ---------------------------------------------------------------------------------------------
# 2. `want` follows needs_input_grad
# ---------------------------------------------------------------------------------------------
def test_want_follows_needs_input_grad(use, monkeypatch):
    p = bases()
    seen = spy_backward(monkeypatch)
    be = use(SharedOracleBackend())
    lv = leaves_of(p, no_grad=("c", "F", "f"))
    got = step_grads(p, lv, [lv[k] for k in NAMES], True, shared_grad_kernel=True)
    assert be.wants == [(True, False, False, False)]
    r = be.returned[0]
    assert r["sum_dC"] == (T, N, N) and r["sum_dc"] is None and r["sum_dF"] is None and r["sum_df"] is None
    assert seen == [[None, (B, NS), (T, N, N), None, None, None]]
    use(OracleBackend())
    lr = leaves_of(p, no_grad=("c", "F", "f"))
    assert_close(got, step_grads(p, lr, views(lr), True))


# ---------------------------------------------------------------------------------------------
# 1b. routing: mpc.MPC
# ---------------------------------------------------------------------------------------------
def mpc_grads(p, leaves, args, n_batch=B, **kw):
    ctrl = mpc.MPC(NS, NC, T, u_lower=-0.4, u_upper=0.4, lqr_iter=6, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                   n_batch=n_batch, **kw)
    x, u, _ = ctrl(p["x_init"], QuadCost(args[0], args[1]), LinDx(args[2], args[3]))
    loss = (x * p["wx"]).sum() + (u * p["wu"]).sum()
    return torch.autograd.grad(loss, [leaves[k] for k in NAMES if leaves[k].requires_grad]), x.detach(), u.detach()


@pytest.mark.parametrize("time_invariant", (False, True))
def test_mpc_takes_the_summed_route_for_a_shared_cost_and_model(use, monkeypatch, time_invariant):
    p = bases(time_invariant)
    seen = spy_backward(monkeypatch)
    be = use(SharedOracleBackend())
    lv = leaves_of(p)
    got, x, u = mpc_grads(p, lv, [lv[k] for k in NAMES], shared_grad_kernel=True)
    assert be.calls.count("kkt_backward_shared") == 1 and "kkt_backward" not in be.calls
    assert seen == [[None, (B, NS)] + [tuple(p[k].shape) for k in NAMES]]
    ref_be = use(OracleBackend())
    lr = leaves_of(p)
    ref, xr, ur = mpc_grads(p, lr, views(lr))
    assert ref_be.calls.count("kkt_backward") == 1
    assert torch.equal(x, xr) and torch.equal(u, ur)                 # the iterations are untouched
    assert_close(got, ref)
    # the flag off with the same shared forms: the cost's (and now the model's) views, autograd's sum -- the parent's route
    off_be = use(SharedOracleBackend())
    lo = leaves_of(p)
    off, xo, uo = mpc_grads(p, lo, [lo[k] for k in NAMES])
    assert "kkt_backward_shared" not in off_be.calls and off_be.calls.count("kkt_backward") == 1
    assert torch.equal(xo, xr) and torch.equal(uo, ur)
    assert_close(off, ref)


@pytest.mark.parametrize("case", ("full_rank_C", "slew", "reference_du_norm", "no_method"))
def test_mpc_declining_cases_keep_the_per_problem_route(use, case):
    p = bases()
    kw = dict(slew=dict(slew_rate_penalty=0.3), reference_du_norm=dict(reference_du_norm=True)).get(case, {})
    full = ("C",) if case == "full_rank_C" else ()
    use(OracleBackend())
    lr = leaves_of(p, full=full)
    ref, xr, ur = mpc_grads(p, lr, views(lr), **kw)
    be = use(OracleBackend() if case == "no_method" else SharedOracleBackend())
    lv = leaves_of(p, full=full)
    got, x, u = mpc_grads(p, lv, [lv[k] for k in NAMES], shared_grad_kernel=True, **kw)
    assert "kkt_backward_shared" not in be.calls and be.calls.count("kkt_backward") == 1
    assert torch.equal(x, xr) and torch.equal(u, ur)
    assert all(g.shape == lv[k].shape for g, k in zip(got, NAMES))
    assert_close(got, ref)


def test_the_flags_are_off_by_default():
    import inspect
    assert inspect.signature(mpc.MPC.__init__).parameters["shared_grad_kernel"].default is False
    assert inspect.signature(LQRStep).parameters["shared_grad_kernel"].default is False
    assert mpc.MPC(3, 1, 4).shared_grad_kernel is False and mpc.MPC(3, 1, 4, shared_grad_kernel=True).shared_grad_kernel is True
    assert hasattr(_native.HipBackend, "kkt_backward_shared")


# ---------------------------------------------------------------------------------------------
# 3. LinDx in 2- and 3-dimensional form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time_invariant", (False, True))
@pytest.mark.parametrize("with_f", (True, False))
def test_lindx_in_shared_form_solves_bitwise_like_its_expanded_views(use, time_invariant, with_f):
    p = bases(time_invariant)
    use(OracleBackend())
    f = p["f"] if with_f else None
    Cv, cv, Fv, fv = views(p)

    def solve(cost, dx, n_batch):
        ctrl = mpc.MPC(NS, NC, T, u_lower=-0.4, u_upper=0.4, lqr_iter=6, verbose=-1, exit_unconverged=False, n_batch=n_batch)
        with torch.no_grad():
            return ctrl(p["x_init"], cost, dx)
    ref = solve(QuadCost(Cv, cv), LinDx(Fv, fv if with_f else None), None)
    got = solve(QuadCost(p["C"], p["c"]), LinDx(p["F"], f), B)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    # the batch size comes from a full-rank cost as before, whatever the model's form
    got = solve(QuadCost(Cv, cv), LinDx(p["F"], f), None)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    with pytest.raises(ValueError, match="Could not infer batch size"):
        solve(QuadCost(p["C"], p["c"]), LinDx(p["F"], f), None)


def test_lindx_of_the_wrong_rank_is_refused(use):
    p = bases()
    use(OracleBackend())
    with pytest.raises(ValueError, match="LinDx"):
        mpc.MPC(NS, NC, T, n_batch=B, verbose=-1)(p["x_init"], QuadCost(p["C"], p["c"]), LinDx(p["F"][0, 0], None))


# ---------------------------------------------------------------------------------------------
# 4. the C entry without a GPU
# ---------------------------------------------------------------------------------------------
def problem(B_=8, T_=5, ns=12, nc=4, dtype=_native.MPC_F32, F=16):
    p = _native.Problem()
    p.B, p.T, p.ns, p.nc, p.dtype = B_, T_, ns, nc, dtype
    p.x_init = p.C = p.c = p.cur_x = p.cur_u = 16          # never dereferenced: every check below fails before a launch
    if F:
        p.F = F
    p.C_st, p.C_sb, p.c_st, p.c_sb, p.F_st, p.F_sb = 0, 0, 0, 0, 0, 0
    return p


def test_entry_point_validates_arguments_without_gpu():
    L = _native.load()
    E_DIMS, E_NULL, E_ARG = -1, -2, -5

    def call(p, *a):          # a: dx, du, dl_dx, dl_du, sum_dC, sum_dc, sum_dF, sum_df, dx_init, workspace, bytes
        a = list(a) + [None] * (10 - len(a)) + ([0] if len(a) < 11 else [])
        return L.mpc_lqr_kkt_grads_shared(None if p is None else ctypes.byref(p), *a[:10], a[10], None)
    p = problem()
    need = L.mpc_lqr_kkt_shared_workspace_bytes(ctypes.byref(p))
    assert L.mpc_lqr_kkt_shared_supported(ctypes.byref(p)) == 1 and need > 0 and need % 16 == 0
    ok = [16] * 4 + [None] * 4 + [16]                       # the four inputs, no sums wanted, dx_init
    assert call(None) == E_NULL
    assert call(p) == E_NULL                                                      # dx NULL
    assert call(p, 16, 16, 16, 16, None, None, None, None, None, 16, need) == E_NULL      # dx_init NULL
    assert call(p, *ok, None, need) == E_NULL and b"workspace" in L.mpc_lqr_last_error()
    assert call(problem(F=0), *ok, 16, need) == E_NULL                            # F NULL with T > 1
    assert call(p, *ok, 16, need - 1) == E_DIMS and b"workspace" in L.mpc_lqr_last_error()
    assert call(p, *ok, 20, need + 16) == E_ARG and b"aligned" in L.mpc_lqr_last_error()
    p64 = problem(dtype=_native.MPC_F64)
    assert L.mpc_lqr_kkt_shared_supported(ctypes.byref(p64)) == 0 and L.mpc_lqr_kkt_shared_workspace_bytes(ctypes.byref(p64)) == 0
    assert call(p64, *ok, 16, 1 << 30) == E_DIMS and b"float32" in L.mpc_lqr_last_error()
    p65 = problem(ns=45, nc=20)
    assert L.mpc_lqr_kkt_shared_supported(ctypes.byref(p65)) == 0
    assert call(p65, *ok, 16, 1 << 30) == E_DIMS
    assert L.mpc_lqr_kkt_shared_supported(ctypes.byref(problem(ns=45, nc=19))) == 1
    assert L.mpc_lqr_kkt_shared_supported(ctypes.byref(problem(ns=63, nc=1))) == 1
    assert call(problem(B_=0)) == 0                                               # nothing to do, nothing looked at
    assert call(problem(B_=-1), *ok, 16, need) == E_DIMS
    # the workspace: the compact costates [T-1,B,2 ns] and at most MPC_KKT_SHARED_MAX_PARTIALS partials per timestep
    words = 16 * 16 + 12 * 16 + 16 + 12
    for B_, T_, parts in ((1, 1, 1), (3, 9, 1), (67, 9, 3), (1030, 9, 32), (4096, 50, 21), (10 ** 6, 2, 32)):
        q = problem(B_=B_, T_=T_)
        costates = ((T_ - 1) * B_ * 24 * 4 + 15) // 16 * 16
        assert L.mpc_lqr_kkt_shared_workspace_bytes(ctypes.byref(q)) == costates + T_ * parts * words * 4


def test_exports_are_the_header_s_declarations():
    header = open(os.path.join(ROOT, "include", "mpc_lqr.h")).read()
    declared = set(re.findall(r"\b(mpc_[a-z_]+)\s*\(", header))
    assert {"mpc_lqr_kkt_shared_supported", "mpc_lqr_kkt_shared_workspace_bytes", "mpc_lqr_kkt_grads_shared"} <= declared
    assert set(_native.EXPORTS) == declared
    assert re.search(r"#define MPC_LQR_ABI_VERSION 9\b", header) and _native.load().mpc_lqr_abi_version() == 9
