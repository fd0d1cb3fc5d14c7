"""CPU-only: impl 10 (MPC_IMPL_WAVE1_CARRY, the row-per-problem kernel for a simulator behind MPC_ENV_CTRL_CARRY) in the host-side
decisions -- mpc_lqr_impl_supported, mpc_lqr_step_route for a forced 10 and what impl 0 and impl 6 keep answering,
mpc_lqr_row_carry_pays against the LDS arithmetic written out here -- and `MPC(row_carry_kernel=True)` on a spying stand-in backend.
No call here reaches a launch; every pointer of the C calls is made up (the queries dereference none)."""
import ctypes
import importlib.util
import os

import pytest
import torch

from conftest import GOLDEN
from mpc import _native, mpc
from mpc.env_dx import cartpole, pendulum
from mpc.mpc import GradMethods, LinDx, QuadCost
from oracle_backend import OracleBackend

_spec = importlib.util.spec_from_file_location("make_golden_step_route", os.path.join(GOLDEN, "make_golden_step_route.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
ROW_CARRY, TINY, WAVE1 = 10, 4, 6
CARRY = gen.ENV_CTRL_CARRY
PENDULUM, PENDULUM_FULL, CARTPOLE = 1, 2, 3
E_DIMS, E_DTYPE, E_ARG, E_UNSUPPORTED = -1, -3, -5, -6
r = ctypes.byref


@pytest.fixture
def lib():
    _native.load()
    L = gen.bind(_native)
    L.mpc_lqr_step_route.argtypes = L.mpc_lqr_step.argtypes[:6] + [ctypes.POINTER(ctypes.c_int)]
    L.mpc_lqr_row_carry_pays.argtypes = L.mpc_lqr_impl_supported.argtypes[:2]
    return L


def test_the_python_constant_is_the_c_one_and_the_abi_is_where_it_was(lib):
    assert _native.IMPL_WAVE1_CARRY == ROW_CARRY
    assert int(lib.mpc_lqr_abi_version()) == _native.ABI_VERSION == 9
    assert b"lqr_step_wave1_carry<f32>" in _native.load().mpc_lqr_build_info()
    assert (_native.MPC_F32, E_DIMS, E_DTYPE, E_ARG, E_UNSUPPORTED) == (0, -1, -3, -5, -6)


def supported(L, ns, nc, o, dtype=None, impl=ROW_CARRY, T=5, B=3):
    p = gen.problem(_native, ns, nc, _native.MPC_F32 if dtype is None else dtype, T, B)
    return int(L.mpc_lqr_impl_supported(r(p), None if o is None else r(o), impl))


def test_impl_supported_takes_the_two_augmented_simulators_in_float32_and_nothing_else(lib):
    for kind, ns in ((PENDULUM, 4), (PENDULUM_FULL, 4), (CARTPOLE, 6)):
        for lin in (0, 1):
            for box in (0, 1, 2):
                o, _e = gen.options(_native, box=box, env=(kind | CARRY, lin))
                assert supported(lib, ns, 1, o) == 1, (kind, lin, box)
                assert supported(lib, ns, 1, o, dtype=_native.MPC_F64) == 0
                assert supported(lib, ns, 1, o, impl=TINY) == 1 and supported(lib, ns, 1, o, impl=WAVE1) == 0      # as ever
        o, _e = gen.options(_native, env=(kind | CARRY, 1), max_ls=16)
        assert supported(lib, ns, 1, o) == 1
        o, _e = gen.options(_native, env=(kind | CARRY, 1), max_ls=17)
        assert supported(lib, ns, 1, o) == 0
        o, _e = gen.options(_native, env=(kind | CARRY, 1))
        assert supported(lib, ns - 1, 1, o) == 0                         # 3 / 1 and 5 / 1: not the augmented sizes
        assert supported(lib, ns, 1, o, T=2000) == 0                     # four problems no longer fit 150 KiB of LDS
        o, _e = gen.options(_native, env=(kind, 1))
        assert supported(lib, ns - 1, 1, o) == 0                         # a plain simulator (impl 6 has it)
        assert supported(lib, ns - 1, 1, o, impl=WAVE1) == 1
        o, _e = gen.options(_native, env=(kind | CARRY, 0), flags=gen.OPT_SWEEP_ONLY)
        assert supported(lib, ns, 1, o) == 0                             # a whole step only
    for ns in (3, 4, 6):
        assert supported(lib, ns, 1, None) == 0 and supported(lib, ns, 1, gen.options(_native)[0]) == 0     # no simulator at all
    assert supported(lib, 4, 1, gen.options(_native)[0], impl=ROW_CARRY + 1) == 0


def route(L, ns, impl, o, dtype=None, T=5, B=3, ws="full"):
    p = gen.problem(_native, ns, 1, _native.MPC_F32 if dtype is None else dtype, T, B)
    out = gen.outputs(_native)
    full = int(L.mpc_lqr_workspace_bytes(r(p)))
    w, nbytes = {"full": (gen.WS, full), "none": (None, 0)}[ws]
    ring = ctypes.c_int(-1)
    rc = int(L.mpc_lqr_step_route(r(p), r(o), r(out), w, nbytes, impl, r(ring)))
    return rc, L.mpc_lqr_last_error().decode()


def test_step_route_answers_10_for_a_forced_10_and_4_for_auto_at_every_batch(lib):
    for kind, ns in ((PENDULUM, 4), (PENDULUM_FULL, 4), (CARTPOLE, 6)):
        for lin in (0, 1):
            o, _e = gen.options(_native, box=1, env=(kind | CARRY, lin))
            for B in (8, 100000):
                assert route(lib, ns, ROW_CARRY, o, B=B)[0] == ROW_CARRY
                assert route(lib, ns, 0, o, B=B)[0] == TINY
                assert route(lib, ns, TINY, o, B=B)[0] == TINY
            rc, msg = route(lib, ns, WAVE1, o, B=8)
            assert rc == E_UNSUPPORTED and "MPC_ENV_CTRL_CARRY" in msg
            for impl in (1, 2, 3, 5, 7, 8, 9):
                assert route(lib, ns, impl, o)[0] == E_UNSUPPORTED, impl


def test_a_forced_10_is_refused_with_a_code_and_a_text_of_its_own(lib):
    carry, _e1 = gen.options(_native, box=1, env=(PENDULUM | CARRY, 1))
    assert route(lib, 4, ROW_CARRY, carry, dtype=_native.MPC_F64) == (E_DTYPE, "the row-per-problem carry kernel is fp32 only")
    plain, _e2 = gen.options(_native, box=1, env=(PENDULUM, 1))
    needs = "the row-per-problem carry kernel needs a simulator behind MPC_ENV_CTRL_CARRY as true_dynamics"
    assert route(lib, 3, ROW_CARRY, plain) == (E_ARG, needs)
    assert route(lib, 3, ROW_CARRY, gen.options(_native, box=1)[0]) == (E_ARG, needs)               # a linear model
    assert route(lib, 4, ROW_CARRY, gen.options(_native)[0]) == (E_ARG, needs)
    rc, msg = route(lib, 7, ROW_CARRY, gen.options(_native)[0])
    assert rc == E_DIMS and msg.startswith("the row-per-problem carry kernel needs a whole step with n_ctrl = 1")
    rc, msg = route(lib, 3, ROW_CARRY, carry)                                                       # sizes that are not the augmented ones
    assert rc == E_DIMS and msg == "n_state / n_ctrl do not match the simulator"
    limits = "the row-per-problem carry kernel is float32, max_linesearch_iter <= 16, four problems in 150 KiB of LDS"
    ls17, _e3 = gen.options(_native, box=1, env=(PENDULUM | CARRY, 1), max_ls=17)
    assert route(lib, 4, ROW_CARRY, ls17) == (E_DIMS, limits)
    assert route(lib, 4, ROW_CARRY, carry, T=2000) == (E_DIMS, limits)
    rc, msg = route(lib, 4, ROW_CARRY, carry, ws="none")
    assert rc == E_ARG and msg.startswith("workspace too small")
    sweep, _e4 = gen.options(_native, env=(PENDULUM | CARRY, 0), flags=gen.OPT_SWEEP_ONLY)
    rc, msg = route(lib, 4, ROW_CARRY, sweep)
    assert rc == E_ARG and msg.startswith("MPC_OPT_SWEEP_ONLY")
    sweep, _e5 = gen.options(_native, flags=gen.OPT_SWEEP_ONLY)
    rc, msg = route(lib, 4, ROW_CARRY, sweep)
    assert rc == E_ARG and msg.startswith("MPC_OPT_SWEEP_ONLY")


# ---------------------------------------------------------------------------------------------
# mpc_lqr_row_carry_pays: wave1::layout's arithmetic (csrc/lqr_wave1_body.h), written out
# ---------------------------------------------------------------------------------------------
def lds_floats(ns, T, ntrial, bounded):
    """one problem's share of the LDS in floats: C, c, C tau + c (the gains later), F, the nominal, the bounds, every trial's trajectory;
    no f (a simulator has none), no mask"""
    N = ns + 1
    return T * N * N + T * N + T * N + T * ns * N + T * N + (2 * T if bounded else 0) + ntrial * T * N


def last_paying_batch(ns, T, ntrial, bounded, simds=1024):
    """auto's rule for impl 6 on these bytes: every wavefront (four problems, 16 bytes a float-slot) resident at once -- as many to a
    CU (four SIMDs) as 160 KiB hold, eight at the most"""
    per_wave = lds_floats(ns, T, ntrial, bounded) * 16
    per_cu = min((160 * 1024) // per_wave, 8)
    return 4 * (simds // 4) * per_cu, per_wave


def pays(L, kind, ns, T, B, box=1, max_ls=10, dtype=None, flags=0, carry=CARRY, lin=1):
    p = gen.problem(_native, ns, 1, _native.MPC_F32 if dtype is None else dtype, T, B)
    if lin:
        p.F = None                # (a linearising simulator has no F)
    o, _e = gen.options(_native, box=box, max_ls=max_ls, flags=flags, env=(kind | carry, lin))
    return int(L.mpc_lqr_row_carry_pays(r(p), r(o)))


def test_row_carry_pays_is_the_row_kernels_rule_on_the_carry_kernels_lds(lib):
    assert lds_floats(4, 20, 10, True) == 2240 and lds_floats(6, 25, 10, True) == 4600
    assert last_paying_batch(4, 20, 10, True) == (4096, 35840)          # four wavefronts a CU
    assert last_paying_batch(6, 25, 10, True) == (2048, 73600)          # two
    for kind, ns, T in ((PENDULUM, 4, 20), (PENDULUM_FULL, 4, 20), (CARTPOLE, 6, 25)):
        for box, max_ls in ((1, 10), (0, 10), (2, 3), (1, 16), (1, 1)):
            last, _ = last_paying_batch(ns, T, max_ls, box != 0)
            got = [pays(lib, kind, ns, T, B, box=box, max_ls=max_ls) for B in (1, last - 3, last, last + 1, 2 * last)]
            assert got == [1, 1, 1, 0, 0], (kind, box, max_ls, last, got)
    assert pays(lib, PENDULUM, 4, 20, 4096) == 1 and pays(lib, PENDULUM, 4, 20, 4097) == 0
    assert pays(lib, CARTPOLE, 6, 25, 2048) == 1 and pays(lib, CARTPOLE, 6, 25, 2049) == 0
    assert pays(lib, PENDULUM, 4, 20, 64, lin=0) == 1                   # the caller's augmented F instead of the kernel's own


def test_row_carry_pays_answers_0_wherever_impl_10_refuses_and_says_nothing(lib):
    lib.mpc_lqr_impl_supported(None, None, 1)
    p = gen.problem(_native, 4, 1, 7, 5, 3)
    assert lib.mpc_lqr_workspace_bytes(r(p)) >= 0
    o, _e = gen.options(_native, env=(PENDULUM | CARRY, 1))
    assert int(lib.mpc_lqr_step_route(r(p), r(o), r(gen.outputs(_native)), gen.WS, 1 << 20, 0, None)) == E_DTYPE
    before = lib.mpc_lqr_last_error()
    assert before
    assert pays(lib, PENDULUM, 4, 20, 8, dtype=_native.MPC_F64) == 0
    assert pays(lib, PENDULUM, 4, 20, 8, max_ls=17) == 0
    assert pays(lib, PENDULUM, 4, 20, 8, carry=0) == 0                  # sizes against the plain simulator
    assert pays(lib, PENDULUM, 3, 20, 8, carry=0) == 0                  # a plain simulator
    assert pays(lib, PENDULUM, 3, 20, 8) == 0                           # the flag at the plain sizes
    assert pays(lib, CARTPOLE, 4, 20, 8) == 0
    assert pays(lib, PENDULUM, 4, 20, 8, flags=gen.OPT_SWEEP_ONLY) == 0
    assert pays(lib, PENDULUM, 4, 20, 0) == 0
    assert pays(lib, PENDULUM, 4, 2000, 8) == 0
    p = gen.problem(_native, 4, 1, _native.MPC_F32, 20, 8)
    assert int(lib.mpc_lqr_row_carry_pays(r(p), r(gen.options(_native, box=1)[0]))) == 0       # no simulator
    assert int(lib.mpc_lqr_row_carry_pays(r(p), None)) == 0 and int(lib.mpc_lqr_row_carry_pays(None, None)) == 0
    assert lib.mpc_lqr_last_error() == before                           # silent
    be = _native.HipBackend()
    env = pendulum.PendulumDx().native_env().augmented()
    env.linearize = True
    opts = _native.StepOptions(u_lower=-2.0, u_upper=2.0, true_dynamics=env)
    assert be.row_carry_pays(4, 1, torch.float32, 20, 4096, opts) is True and be.row_carry_pays(4, 1, torch.float32, 20, 4097, opts) is False
    assert be.row_carry_pays(4, 1, torch.float64, 20, 8, opts) is False
    env6 = cartpole.CartpoleDx().native_env().augmented()
    assert be.row_carry_pays(6, 1, torch.float32, 25, 2048, _native.StepOptions(u_lower=-1.0, u_upper=1.0, true_dynamics=env6)) is True


# ---------------------------------------------------------------------------------------------
# MPC(row_carry_kernel=...) on a stand-in backend that records the impl of every plan
# ---------------------------------------------------------------------------------------------
class SpyWithoutTheQuery(OracleBackend):
    """Says it carries the control (so the slew-rate solve around a simulator takes the device-side loop), records what it is asked and
    the `impl` keyword of every plan, and answers every carry step with the nominal it was given -- the loop stops after one iteration.
    supports: what `impl_supported(.., 10, ..)` says.  This one has no `row_carry_pays`; SpyBackend below does."""

    def __init__(self, supports=True, pays=True):
        super().__init__()
        self.supports, self.pays, self.asked, self.plans = supports, pays, [], []

    def impl_supported(self, ns, nc, dtype, impl, opts=None):
        self.asked.append(("impl_supported", ns, nc, impl))
        if impl == TINY:
            return opts is not None and opts.true_dynamics is not None and opts.true_dynamics.carry and ns in (4, 6)
        return impl == ROW_CARRY and self.supports

    def env_traj_cost(self, x_init, u, env, C=None, c=None, want_x=True):
        assert env.carry
        return x_init.unsqueeze(0).expand(u.shape[0], -1, -1).contiguous(), None

    def plan_step(self, x_init, C, c, F, f, cur_x, cur_u, opts, out_x=None, out_u=None, **kw):
        self.plans.append((x_init.shape[1], C.shape[2] - x_init.shape[1], kw))
        if opts.true_dynamics is None:
            return super().plan_step(x_init, C, c, F, f, cur_x, cur_u, opts, out_x=out_x, out_u=out_u, **kw)
        B = x_init.shape[0]

        def run():
            out_x.copy_(cur_x); out_u.copy_(cur_u)
            z = torch.zeros(B, dtype=C.dtype)
            return dict(new_x=out_x, new_u=out_u, costs=z, old_costs=z, full_du_norm=z, alpha_du_norm=z, alphas=z + 1,
                        qp_iters=torch.zeros(B, dtype=torch.int32), status=torch.zeros(B, dtype=torch.int32))
        return run


class SpyBackend(SpyWithoutTheQuery):
    def row_carry_pays(self, ns, nc, dtype, T, B, opts, like=None):
        self.asked.append(("row_carry_pays", ns, nc, T, B))
        return self.pays


def sim_solve(be, flag, dtype=torch.float32, kind="pendulum", T=5, B=3):
    dx = pendulum.PendulumDx() if kind == "pendulum" else cartpole.CartpoleDx()
    ns = dx.n_state
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(B, ns, generator=g).to(dtype)
    n = ns + 1
    C = torch.eye(n, dtype=dtype).expand(T, B, n, n).contiguous()
    c = torch.zeros(T, B, n, dtype=dtype)
    prev = _native.set_backend_for_testing(be)
    try:
        kw = dict(row_carry_kernel=True) if flag else {}
        ctrl = mpc.MPC(ns, 1, T, u_lower=-1.0, u_upper=1.0, lqr_iter=3, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                       backprop=False, grad_method=GradMethods.ANALYTIC, slew_rate_penalty=0.5, **kw)
        with torch.no_grad():
            be.result = ctrl(x0, QuadCost(C, c), dx)
    finally:
        _native.set_backend_for_testing(prev)
    return be.plans


def asked_about_10(be):
    return [a for a in be.asked if a[0] == "row_carry_pays" or a[3] == ROW_CARRY]


def test_the_flag_binds_impl_10_where_both_predicates_hold():
    for kind, ns in (("pendulum", 4), ("cartpole", 6)):
        be = SpyBackend()
        plans = sim_solve(be, True, kind=kind)
        assert plans and all(pl == (ns, 1, dict(impl=ROW_CARRY)) for pl in plans), plans
        # ... asked at the sizes the loop runs at: the augmented state, the horizon, the batch
        assert ("impl_supported", ns, 1, ROW_CARRY) in be.asked and ("row_carry_pays", ns, 1, 5, 3) in be.asked
        assert be.result[0].shape == (5, 3, ns - 1)


def test_the_flag_binds_no_impl_where_a_predicate_fails_or_the_dtype_is_float64_or_the_dynamics_are_linear():
    for be in (SpyBackend(supports=False), SpyBackend(pays=False), SpyWithoutTheQuery()):
        plans = sim_solve(be, True)
        assert plans and all(pl == (4, 1, {}) for pl in plans), plans
    be = SpyBackend()
    plans = sim_solve(be, True, dtype=torch.float64)
    assert plans and all(pl == (4, 1, {}) for pl in plans) and not asked_about_10(be)
    # a LinDx slew solve (3 / 1 becomes 4 / 1): no simulator, nothing asked, no impl
    be = SpyBackend()
    prev = _native.set_backend_for_testing(be)
    try:
        g = torch.Generator().manual_seed(3)
        T, B, ns = 4, 2, 3
        L = torch.randn(T, B, 4, 4, generator=g)
        C = L @ L.transpose(2, 3) / 4 + torch.eye(4)
        F = 0.1 * torch.randn(T - 1, B, ns, 4, generator=g) + torch.cat((torch.eye(ns), torch.zeros(ns, 1)), 1)
        ctrl = mpc.MPC(ns, 1, T, u_lower=-1.0, u_upper=1.0, lqr_iter=2, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                       backprop=False, slew_rate_penalty=1.0, row_carry_kernel=True)
        with torch.no_grad():
            ctrl(torch.randn(B, ns, generator=g), QuadCost(C, torch.randn(T, B, 4, generator=g)), LinDx(F, 0.1 * torch.randn(T - 1, B, ns, generator=g)))
    finally:
        _native.set_backend_for_testing(prev)
    assert be.plans and all(pl == (4, 1, {}) for pl in be.plans) and not asked_about_10(be)


def test_flag_off_asks_neither_predicate():
    be = SpyBackend()
    plans = sim_solve(be, False)
    assert plans and all(pl == (4, 1, {}) for pl in plans) and not asked_about_10(be)
    assert mpc.MPC(3, 1, 4).row_carry_kernel is False
    on = SpyBackend(pays=False)
    sim_solve(on, True)
    for a, b in zip(on.result, be.result):
        assert torch.equal(a, b)
