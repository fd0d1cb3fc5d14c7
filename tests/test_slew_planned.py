"""CPU tests of the device-side slew-rate loop (round 11): the control carry of the shipped simulators compiled for the host
(csrc/env_dynamics.h env_step_carry, csrc/lqr_tiny_body.h) against mpc.dynamics.CtrlPassthroughDynamics around the package's own
simulators, MPC's routing (`MPC._slew_plan` / `_iterate_slew`) on the CPU stand-in against the route-off solve and the
reference-made fixture, and the argument checks of mpc_slew_augment."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from mpc import _native, mpc
from mpc.dynamics import CtrlPassthroughDynamics
from mpc.env_dx import cartpole, pendulum
from mpc.mpc import GradMethods, LinDx, QuadCost
from oracle_backend import OracleBackend

CSRC = os.path.join(ROOT, "mpc.pytorch_amd", "csrc")

HARNESS = r"""
#include "lqr_tiny_body.h"
using namespace mpclqr;

static EnvDesc<double> desc(int kind, const double *prm, double dt, double u_max, int linearize, int carry)
{
    EnvDesc<double> e;
    e.kind = kind; e.linearize = linearize; e.params = prm; e.dt = dt; e.u_max = u_max; e.carry = carry;
    return e;
}

// N carry transitions z [N, ns+1], u [N] -> out [N, ns+1], J [N, ns+1, ns+2]; and the plain transition's Jacobian Je [N, ns, ns+1]
extern "C" void carry_points(int kind, const double *prm, double dt, double u_max, long N, const double *z, const double *u,
                             double *out, double *J, double *out_nojac, double *Je)
{
    const EnvDesc<double> e = desc(kind, prm, dt, u_max, 0, 1);
    const int ns = env_ns(kind), n = ns + 1, na = ns + 2;
    for (long i = 0; i < N; ++i) {
        double xe[5];
        if (ns == 5) {
            env_step_carry<double, 5>(e, z + i * n, u[i], out + i * n, J + i * n * na);
            env_step_carry<double, 5>(e, z + i * n, u[i], out_nojac + i * n, nullptr);
        } else {
            env_step_carry<double, 3>(e, z + i * n, u[i], out + i * n, J + i * n * na);
            env_step_carry<double, 3>(e, z + i * n, u[i], out_nojac + i * n, nullptr);
        }
        env_step<double>(e, z + i * n + 1, u[i], xe, Je + i * ns * n);
    }
}

// one LQR step of the lane-per-problem body, every problem on one host "lane": the simulator behind the carry as the true
// dynamics of the rollout; the sweep's model from the body's own linearisation (F == nullptr) or from the caller's F
template <int NS>
static void step(int kind, const double *prm, double dt, double u_max, int T, int B, const double *x_init, const double *C,
                 const double *c, const double *F, const double *cur_x, const double *cur_u, double lo, double hi, int max_ls,
                 double decay, double *new_x, double *new_u, double *costs, double *alphas, double *K, double *k, double *ws)
{
    constexpr int N = NS + 1;
    StepParams<double> p = StepParams<double>();
    p.B = B; p.T = T; p.ns = NS; p.nc = 1;
    p.x_init = x_init; p.C = C; p.c = c; p.F = F; p.f = nullptr; p.cur_x = cur_x; p.cur_u = cur_u;
    p.C_st = (long)B * N * N; p.C_sb = N * N; p.c_st = (long)B * N; p.c_sb = N; p.F_st = (long)B * NS * N; p.F_sb = NS * N;
    p.bound_mode = MPC_BOUND_SCALAR; p.lo_s = lo; p.hi_s = hi;
    p.ls_decay = decay; p.max_ls = max_ls; p.pnqp_iter = 20;
    p.new_x = new_x; p.new_u = new_u; p.costs = costs; p.alphas = alphas; p.K = K; p.k = k;
    p.env = desc(kind, prm, dt, u_max, F == nullptr, 1);
    double *Kw = ws, *Tw = ws + (long)T * N * B;
    for (int b = 0; b < B; ++b) tiny::lqr_step_problem<double, NS>(p, b, Kw, Tw, tiny::OneLane());
}
extern "C" void carry_step(int kind, const double *prm, double dt, double u_max, int T, int B, const double *x_init,
                           const double *C, const double *c, const double *F, const double *cur_x, const double *cur_u, double lo,
                           double hi, int max_ls, double decay, double *new_x, double *new_u, double *costs, double *alphas,
                           double *K, double *k, double *ws)
{
    if (env_ns(kind) == 5) step<6>(kind, prm, dt, u_max, T, B, x_init, C, c, F, cur_x, cur_u, lo, hi, max_ls, decay, new_x, new_u, costs, alphas, K, k, ws);
    else step<4>(kind, prm, dt, u_max, T, B, x_init, C, c, F, cur_x, cur_u, lo, hi, max_ls, decay, new_x, new_u, costs, alphas, K, k, ws);
}
"""

SIMS = {"pendulum": lambda: pendulum.PendulumDx(), "pendulum_full": lambda: pendulum.PendulumDx(simple=False),
        "cartpole": lambda: cartpole.CartpoleDx()}


def make_sim(kind):
    dx = SIMS[kind]()
    dx.params = dx.params.double()
    return dx


def sim_points(dx, N, seed, u_scale):
    """N augmented points (u_prev, x) and controls, a few of them outside the simulator's clamp."""
    g = torch.Generator().manual_seed(seed)
    th = (torch.rand(N, generator=g, dtype=torch.float64) - 0.5) * 2.5
    w = torch.randn(N, generator=g, dtype=torch.float64)
    if dx.n_state == 3:
        x = torch.stack((th.cos(), th.sin(), w), 1)
    else:
        r = 0.5 * torch.randn(N, 2, generator=g, dtype=torch.float64)
        x = torch.stack((r[:, 0], r[:, 1], th.cos(), th.sin(), w), 1)
    u = u_scale * torch.randn(N, 1, generator=g, dtype=torch.float64)
    up = torch.randn(N, 1, generator=g, dtype=torch.float64)
    return torch.cat((up, x), 1), u


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """csrc/lqr_tiny_body.h (with env_dynamics.h) compiled for the host, in the test's own temporary directory."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    if not cxx:
        pytest.skip("needs clang++")
    d = tmp_path_factory.mktemp("slew_planned")
    src, so = os.path.join(d, "harness.cpp"), os.path.join(d, "libharness.so")
    with open(src, "w") as fh:
        fh.write(HARNESS)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function",
                           "-I", CSRC, "-o", so, src])
    return ctypes.CDLL(so)


def _c(a):
    return np.ascontiguousarray(a, np.float64)


def run_points(lib, dx, z, u):
    N, n = z.shape
    ns = n - 1
    prm, zz, uu = _c(dx.params.numpy()), _c(z.numpy()), _c(u.numpy().reshape(-1))
    out, J, out2, Je = np.empty((N, n)), np.empty((N, n, n + 1)), np.empty((N, n)), np.empty((N, ns, n))
    vp = ctypes.c_void_p
    lib.carry_points.argtypes = [ctypes.c_int, vp, ctypes.c_double, ctypes.c_double, ctypes.c_long] + [vp] * 6
    lib.carry_points.restype = None
    lib.carry_points(dx._kind, prm.ctypes.data, float(dx.dt), float(dx._u_max), N, zz.ctypes.data, uu.ctypes.data, out.ctypes.data,
                     J.ctypes.data, out2.ctypes.data, Je.ctypes.data)
    return out, J, out2, Je


# ---------------------------------------------------------------------------------------------
# (a) the carry on the host
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(SIMS))
def test_env_step_carry_is_ctrl_passthrough_around_the_simulator(host_lib, kind):
    """Transition at 1e-12, Jacobian at 1e-9 against autograd through CtrlPassthroughDynamics(simulator) in float64 torch; the
    control is carried RAW (some points lie outside the clamp), the carry row is (0 .. 0 1), the u_prev column zero."""
    dx = make_sim(kind)
    z, u = sim_points(dx, 24, 5, 1.5 * dx._u_max)
    assert 2 <= int((u.abs() > dx._u_max).sum()) <= 20
    mod = CtrlPassthroughDynamics(dx)
    out, J, out2, _ = run_points(host_lib, dx, z, u)
    zt, ut = z.clone().requires_grad_(True), u.clone().requires_grad_(True)
    ref = mod(zt, ut)
    np.testing.assert_allclose(out, ref.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.array_equal(out, out2) and np.array_equal(out[:, 0], u.numpy()[:, 0])
    rows = [torch.cat(torch.autograd.grad(ref[:, r].sum(), [zt, ut], retain_graph=True), 1) for r in range(ref.shape[1])]
    np.testing.assert_allclose(J, torch.stack(rows, 1).numpy(), rtol=1e-9, atol=1e-9)
    n = z.shape[1]
    assert (J[:, 0, :n] == 0).all() and (J[:, 0, n] == 1).all() and (J[:, :, 0] == 0).all()


@pytest.mark.parametrize("kind", sorted(SIMS))
@pytest.mark.parametrize("max_ls", [1, 3])
def test_tiny_body_carry_step_equals_the_body_fed_the_augmented_model(host_lib, kind, max_ls):
    """One step of the lane-per-problem body with the carry and its own linearisation == the same body whose sweep is fed the
    explicit augmented F (assembled here from the PLAIN simulator's Jacobian: carry row, zero column, the block inside)."""
    dx = make_sim(kind)
    T, B = 6, 5
    ns = dx.n_state
    NS, N = ns + 1, ns + 2
    g = torch.Generator().manual_seed(11)
    z0, _ = sim_points(dx, B, 7, 1.0)
    cur_u = 0.3 * torch.randn(T, B, 1, generator=g, dtype=torch.float64)
    mod = CtrlPassthroughDynamics(dx)
    xs = [z0]
    for t in range(T - 1):
        xs.append(mod(xs[-1], cur_u[t]))
    cur_x = torch.stack(xs)
    L = torch.randn(T, B, N, N, generator=g, dtype=torch.float64)
    C = L @ L.transpose(2, 3) + 0.5 * torch.eye(N, dtype=torch.float64)
    c = torch.randn(T, B, N, generator=g, dtype=torch.float64)
    _, _, _, Je = run_points(host_lib, dx, cur_x[:-1].reshape(-1, NS), cur_u[:-1].reshape(-1, 1))
    F = np.zeros((T - 1, B, NS, N))
    F[:, :, 0, N - 1] = 1.0
    F[:, :, 1:, 1:] = Je.reshape(T - 1, B, ns, ns + 1)
    bound = 0.4

    def run(Fa):
        a = [_c(t.numpy()) for t in (dx.params, z0, C, c, cur_x, cur_u)]
        o = dict(new_x=np.empty((T, B, NS)), new_u=np.empty((T, B, 1)), costs=np.empty(B), alphas=np.empty(B),
                 K=np.empty((T, B, 1, NS)), k=np.empty((T, B, 1)))
        ws = np.zeros(2 * T * N * B)
        vp = ctypes.c_void_p
        host_lib.carry_step.argtypes = ([ctypes.c_int, vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int] + [vp] * 6
                                        + [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double] + [vp] * 7)
        host_lib.carry_step.restype = None
        host_lib.carry_step(dx._kind, a[0].ctypes.data, float(dx.dt), float(dx._u_max), T, B, a[1].ctypes.data, a[2].ctypes.data,
                            a[3].ctypes.data, None if Fa is None else Fa.ctypes.data, a[4].ctypes.data, a[5].ctypes.data, -bound, bound,
                            max_ls, 0.2, *(o[k].ctypes.data for k in ("new_x", "new_u", "costs", "alphas", "K", "k")), ws.ctypes.data)
        return o
    own, fed = run(None), run(_c(F))
    for key in own:
        np.testing.assert_allclose(own[key], fed[key], rtol=1e-12, atol=1e-12, err_msg=key)
    assert (np.abs(own["new_u"]) == bound).any(), "the bounds must clamp some control"
    np.testing.assert_array_equal(own["new_x"][1:, :, 0], own["new_u"][:-1, :, 0])      # the carried control is the raw one


# ---------------------------------------------------------------------------------------------
# (b) routing on the CPU stand-in
# ---------------------------------------------------------------------------------------------
def lin_solve(z, route, dtype=torch.float64):
    ns, nc, T, B, lqr_iter = (int(v) for v in z["meta"])
    t = lambda k: torch.from_numpy(z[k]).to(dtype)
    ctrl = mpc.MPC(ns, nc, T, u_lower=-float(z["bound"][0]), u_upper=float(z["bound"][0]), lqr_iter=lqr_iter, verbose=-1,
                   exit_unconverged=False, detach_unconverged=False, slew_rate_penalty=float(z["gamma"][0]))
    if not route:
        ctrl._slew_plan = lambda *a, **k: None
    with torch.no_grad():
        return ctrl(t("x_init"), QuadCost(t("C"), t("c")), LinDx(t("F"), t("f")))


@pytest.fixture
def oracle_be():
    be = OracleBackend()
    prev = _native.set_backend_for_testing(be)
    yield be
    _native.set_backend_for_testing(prev)


def test_lindx_slew_solve_new_route_equals_route_off_and_the_reference(oracle_be, monkeypatch):
    z = golden("mpc_slew_lin_f64")
    calls = []
    orig = mpc.MPC._solve_slew_subproblem
    monkeypatch.setattr(mpc.MPC, "_solve_slew_subproblem", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    x, u, costs = lin_solve(z, True)
    assert not calls, "the planned route re-packs nothing per iteration"
    xo, uo, co = lin_solve(z, False)
    assert calls
    np.testing.assert_allclose(u.numpy(), uo.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(x.numpy(), xo.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(costs.numpy(), co.numpy(), rtol=1e-9)
    assert x.shape == xo.shape == z["x"].shape
    np.testing.assert_allclose(u.numpy(), z["u"], rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(x.numpy(), z["x"], rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(costs.numpy(), z["costs"], rtol=2e-4)
    assert (np.abs(np.abs(z["u"]) - float(z["bound"][0])) < 1e-9).sum() >= 3, "the fixture must exercise the box QP"


@pytest.mark.parametrize("prev_rank", [1, 2, 3])
def test_prev_ctrl_of_every_rank_reaches_the_augmented_initial_state(oracle_be, prev_rank):
    z = golden("mpc_slew_lin_f64")
    ns, nc, T, B, _ = (int(v) for v in z["meta"])
    t = lambda k: torch.from_numpy(z[k])
    prev = torch.tensor([0.3, -0.2], dtype=torch.float64)
    prev = {1: prev, 2: prev.expand(B, nc), 3: prev.expand(1, B, nc)}[prev_rank]
    outs = []
    for route in (True, False):
        ctrl = mpc.MPC(ns, nc, T, u_lower=-0.5, u_upper=0.5, lqr_iter=6, verbose=-1, exit_unconverged=False,
                       detach_unconverged=False, slew_rate_penalty=1.0, prev_ctrl=prev)
        if not route:
            ctrl._slew_plan = lambda *a, **k: None
        with torch.no_grad():
            outs.append(ctrl(t("x_init"), QuadCost(t("C"), t("c")), LinDx(t("F"), t("f"))))
    for a, b in zip(*outs):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-9, atol=1e-9)


def test_slew_plan_declines_what_stays_on_the_general_loop(oracle_be):
    z = golden("mpc_slew_lin_f64")
    ns, nc, T, B, _ = (int(v) for v in z["meta"])
    t = lambda k: torch.from_numpy(z[k])
    cost, dx, x0 = QuadCost(t("C"), t("c")), LinDx(t("F"), t("f")), t("x_init")
    mk = lambda **kw: mpc.MPC(ns, nc, kw.pop("T", T), slew_rate_penalty=kw.pop("gamma", 1.0), **kw)
    assert mk()._slew_plan(cost, dx, oracle_be, x0) == "lin"
    assert mk(gamma=None)._slew_plan(cost, dx, oracle_be, x0) is None
    assert mk(T=1)._slew_plan(cost, dx, oracle_be, x0) is None
    assert mk(reference_du_norm=True)._slew_plan(cost, dx, oracle_be, x0) is None
    assert mk(reference_du_norm=True)._slew_plan(cost, dx, oracle_be, x0[:1]) == "lin"
    assert mk()._slew_plan(lambda tau: tau.sum(1), dx, oracle_be, x0) is None


def test_simulator_slew_solve_takes_the_old_route_on_a_backend_without_the_carry(oracle_be, monkeypatch):
    """The CPU stand-in has no `impl_supported` (no kernel that carries the control): the predicate declines and the solve goes
    through _solve_slew_subproblem with the module as true dynamics, as before."""
    dx = make_sim("pendulum")
    T, B = 4, 2
    th = torch.tensor([0.3, -0.8], dtype=torch.float64)
    x0 = torch.stack((th.cos(), th.sin(), 0.2 * th), 1)
    q, p = dx.get_true_obj()
    cost = QuadCost(torch.diag(q.double()).expand(T, B, 4, 4).contiguous(), p.double().expand(T, B, 4).contiguous())
    ctrl = mpc.MPC(3, 1, T, u_lower=dx.lower, u_upper=dx.upper, lqr_iter=2, verbose=-1, exit_unconverged=False,
                   detach_unconverged=False, grad_method=GradMethods.AUTO_DIFF, slew_rate_penalty=0.5)
    assert ctrl._slew_plan(cost, dx, oracle_be, x0) is None
    calls = []
    orig = mpc.MPC._solve_slew_subproblem
    monkeypatch.setattr(mpc.MPC, "_solve_slew_subproblem", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    with torch.no_grad():
        x, u, _ = ctrl(x0, cost, dx)
    assert len(calls) >= 1 and x.shape == (T, B, 3)

    class Carrying(OracleBackend):            # ... and a backend that says it carries the control gets the EnvSpec behind the flag
        def impl_supported(self, ns, nc, dtype, impl, opts=None):
            return impl == _native.IMPL_TINY and ns == 4 and opts.true_dynamics.carry
    env = ctrl._slew_plan(cost, dx, Carrying(), x0)
    assert env is not None and env.carry and env.n_state == 4 and env.kind == _native.ENV_PENDULUM
    ctrl.grad_method = GradMethods.FINITE_DIFF
    assert ctrl._slew_plan(cost, dx, Carrying(), x0) is None


def test_env_spec_augmented_sets_the_flag_in_kind():
    dx = make_sim("cartpole")
    e = dx.native_env()
    a = e.augmented()
    assert (e.n_state, a.n_state, a.carry, e.carry) == (5, 6, True, False)
    s, _ = a.to_struct(torch.empty(0, dtype=torch.float64))
    assert s.kind == _native.ENV_CARTPOLE | _native.ENV_CTRL_CARRY == 0x103
    assert ctypes.sizeof(_native.EnvDynamics) == 32


# ---------------------------------------------------------------------------------------------
# (c) mpc_slew_augment's argument checks (no device: every case returns before a launch)
# ---------------------------------------------------------------------------------------------
def test_slew_augment_argument_checks():
    L = _native.load()
    p = _native.Problem()
    p.B, p.T, p.ns, p.nc, p.dtype = 2, 3, 3, 2, _native.MPC_F64
    buf = (ctypes.c_double * 16)()
    ptr = ctypes.addressof(buf)
    assert L.mpc_slew_augment(ctypes.byref(p), 1.0, ptr, ptr, ptr, ptr, None) == -5           # C is NULL: MPC_E_ARG
    assert b"NULL" in L.mpc_lqr_last_error()
    p.B = 0
    assert L.mpc_slew_augment(ctypes.byref(p), 1.0, None, None, None, None, None) == 0        # B = 0: a no-op
    p.B, p.dtype = 2, 7
    assert L.mpc_slew_augment(ctypes.byref(p), 1.0, ptr, ptr, ptr, ptr, None) == -3           # MPC_E_DTYPE
    p.dtype, p.C, p.c, p.F = _native.MPC_F64, ptr, ptr, ptr
    assert L.mpc_slew_augment(ctypes.byref(p), 1.0, ptr, ptr, None, None, None) == -5         # F without aF
    assert L.mpc_slew_augment(None, 1.0, ptr, ptr, ptr, ptr, None) == -2


def test_carry_is_refused_off_the_lane_per_problem_kernel():
    """mpc_lqr_impl_supported answers 1 for impl 4 only; mpc_env_linearize refuses the flag (MPC_E_UNSUPPORTED = -6)."""
    be = _native.HipBackend()
    dx = make_sim("pendulum")
    opts = _native.StepOptions(true_dynamics=dx.native_env().augmented())
    for dtype in (torch.float32, torch.float64):
        assert be.impl_supported(4, 1, dtype, _native.IMPL_TINY, opts)
        for impl in (1, 2, 3, 5, 6, 7, 8):
            assert not be.impl_supported(4, 1, dtype, impl, opts), impl
        assert not be.impl_supported(3, 1, dtype, _native.IMPL_TINY, opts)          # sizes must be the augmented ones
    plain = _native.StepOptions(true_dynamics=dx.native_env())
    assert be.impl_supported(3, 1, torch.float32, _native.IMPL_TINY, plain) and be.impl_supported(3, 1, torch.float32, _native.IMPL_WAVE1, plain)
    e, _keep = dx.native_env().augmented().to_struct(torch.empty(0, dtype=torch.float64))
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.addressof(buf)
    L = _native.load()
    assert L.mpc_env_linearize(ctypes.byref(e), _native.MPC_F64, 1, ptr, ptr, ptr, ptr, None) == -6
    assert b"MPC_ENV_CTRL_CARRY" in L.mpc_lqr_last_error()
