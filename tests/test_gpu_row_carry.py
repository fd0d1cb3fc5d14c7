"""GPU tests (-m gpu) of impl 10 (MPC_IMPL_WAVE1_CARRY): the row-per-problem kernel for a shipped simulator behind MPC_ENV_CTRL_CARRY.
One step against the lane-per-problem kernel (impl 4) on the same float32 tensors, the refusals on the device, and whole slew-rate
solves with `MPC(row_carry_kernel=True)` against the flag-off solve and the reference-made float64 fixtures.

Tolerances: one step at tests/test_gpu_slew_planned.py's F32 (rtol 1e-3 / atol 1e-4); a problem whose step size differs between the two
float32 kernels is a tie of two trial costs and is left out, at most 15 % of the batch (test_wavefront_per_problem_kernel's cap).  Whole
solves: costs within rtol 1e-3 of the flag-off float32 solve (test_headline_shape_slew_solve_new_route_against_route_off); trajectories
within 2 d0 + 1e-4 of the float64 fixture, d0 the flag-off float32 solve's own distance from it -- the two kernels order their float32 sums
differently and the iLQR loop amplifies that over its <= 10 iterations."""
import numpy as np
import pytest
import torch

from conftest import golden
from mpc import _native, lqr_step, mpc
from mpc._native import StepOptions
from mpc.env_dx import cartpole, pendulum
from mpc.mpc import GradMethods, QuadCost

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = dict(rtol=1e-3, atol=1e-4)
TIE_CAP = 0.15
ROW_CARRY = _native.IMPL_WAVE1_CARRY
FLOATS = ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alpha_du_norm")


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()
    return _native.HipBackend()


def host(t):
    return t.detach().cpu().numpy()


def make_sim(kind, dtype=torch.float32):
    dx = {"pendulum": pendulum.PendulumDx, "cartpole": cartpole.CartpoleDx}[kind]()
    dx.params = dx.params.to(dtype)
    return dx


def sim_states(dx, B, seed):
    g = torch.Generator().manual_seed(seed)
    th = (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * 2.0
    w = 0.5 * torch.randn(B, generator=g, dtype=torch.float64)
    if dx.n_state == 3:
        return torch.stack((th.cos(), th.sin(), w), 1)
    r = 0.2 * torch.randn(B, 2, generator=g, dtype=torch.float64)
    return torch.stack((r[:, 0], r[:, 1], th.cos(), th.sin(), w), 1)


def carry_problem(be, kind, T, B, max_ls):
    """the float32 tensors of test_carry_step_equals_the_route_off_step: the simulator's own objective with the penalty folded in, a
    nominal rolled out through the carried simulator, bounds that clamp"""
    dx = make_sim(kind)
    ns = dx.n_state
    bound, gamma = (0.6, 0.5) if kind == "pendulum" else (1.5, 0.1)
    g = torch.Generator().manual_seed(23 + max_ls)
    x0 = sim_states(dx, B, 9).float().to(DEV)
    u = (0.8 * bound * (2 * torch.rand(T, B, 1, generator=g, dtype=torch.float64) - 1)).float().to(DEV)
    prev = (0.3 * torch.randn(B, 1, generator=g, dtype=torch.float64)).float().to(DEV)
    q, p = dx.get_true_obj()
    Q = torch.diag(q.float()).expand(T, B, ns + 1, ns + 1).contiguous().to(DEV)
    pp = p.float().expand(T, B, ns + 1).contiguous().to(DEV)
    env = dx.native_env().augmented()
    env.linearize = True
    aC, ac, _, _ = be.slew_augment(Q, pp, None, None, ns, 1, gamma)
    z0 = torch.cat((prev, x0), 1).contiguous()
    zs, _ = be.env_traj_cost(z0, u, env)
    opts = StepOptions(u_lower=-bound, u_upper=bound, linesearch_decay=dx.linesearch_decay, max_linesearch_iter=max_ls, true_dynamics=env)
    return z0, aC, ac, zs.contiguous(), u, opts, bound, prev


@pytest.mark.parametrize("kind,T,max_ls", [(k, 8, m) for k in ("pendulum", "cartpole") for m in (1, 3, 10)] + [("pendulum", 1, 10)])
def test_row_carry_step_equals_the_lane_per_problem_step(be, kind, T, max_ls):
    """T = 1: the sweep's terminal step alone, nothing to linearise and nothing to roll through the simulator."""
    B = 37
    z0, aC, ac, zs, u, opts, bound, prev = carry_problem(be, kind, T, B, max_ls)
    plan = be.plan_step(z0, aC, ac, None, None, zs, u, opts, impl=ROW_CARRY)
    assert _native.HipBackend.step_route(plan) == (ROW_CARRY, 0)
    r = {k: v.clone() for k, v in plan().items()}
    lane = be.lqr_step(z0, aC, ac, None, None, zs, u, opts, impl=_native.IMPL_TINY)
    torch.cuda.synchronize()
    same = np.isclose(host(r["alphas"]), host(lane["alphas"]), rtol=1e-6)
    print(kind, T, max_ls, "alphas", sorted(set(host(r["alphas"]).round(6).tolist())), "ties", int((~same).sum()), "on a bound",
          int((r["new_u"].abs() == bound).sum()), "max |du|", float((r["new_u"] - lane["new_u"]).abs().max()))
    assert (~same).mean() <= TIE_CAP, (host(r["alphas"]), host(lane["alphas"]))
    for key in FLOATS:
        a, b = (host(v)[same] if v.dim() == 1 else host(v)[:, same] for v in (r[key], lane[key]))
        np.testing.assert_allclose(a, b, err_msg=key, **F32)
    assert np.array_equal(host(r["status"])[same], host(lane["status"])[same])
    assert int((r["new_u"].abs() == bound).sum()) > 0, "bounds tight enough that some controls clamp"
    assert torch.equal(r["new_x"][1:, :, 0], r["new_u"][:-1, :, 0]) and torch.equal(r["new_x"][0, :, 0], prev[:, 0])
    assert torch.equal(r["new_x"][0], z0)


def test_refusals_on_the_device(be):
    T, B = 4, 3
    for dtype, code, text in ((torch.float64, 3, "fp32 only"), (torch.float32, None, None)):
        dx = make_sim("pendulum", dtype)
        env = dx.native_env().augmented()
        z0 = torch.cat((torch.zeros(B, 1, dtype=dtype), sim_states(dx, B, 1).to(dtype)), 1).to(DEV)
        u = torch.zeros(T, B, 1, dtype=dtype, device=DEV)
        zs, _ = be.env_traj_cost(z0, u, env)
        C = torch.eye(5, dtype=dtype, device=DEV).expand(T, B, 5, 5).contiguous()
        c = torch.zeros(T, B, 5, dtype=dtype, device=DEV)
        F = torch.zeros(T - 1, B, 4, 5, dtype=dtype, device=DEV)
        if code is not None:
            with pytest.raises(RuntimeError, match=r"\(-%d\).*%s" % (code, text)):
                be.lqr_step(z0, C, c, F, None, zs, u, StepOptions(true_dynamics=env), impl=ROW_CARRY)
            continue
        # float32: the carried simulator runs; a linear model (LinDx) and a plain simulator are refused; impl 6 keeps refusing the flag
        r = be.lqr_step(z0, C, c, F, None, zs, u, StepOptions(true_dynamics=env), impl=ROW_CARRY)
        assert torch.isfinite(r["new_x"]).all()
        needs = r"\(-5\).*needs a simulator behind MPC_ENV_CTRL_CARRY"
        with pytest.raises(RuntimeError, match=needs):
            be.lqr_step(z0, C, c, F, None, zs, u, StepOptions(), impl=ROW_CARRY)
        with pytest.raises(RuntimeError, match=needs):
            be.lqr_step(z0[:, 1:].contiguous(), C[:, :, 1:, 1:].contiguous(), c[:, :, 1:].contiguous(), F[:, :, 1:, 1:].contiguous(), None,
                        zs[:, :, 1:].contiguous(), u, StepOptions(true_dynamics=dx.native_env()), impl=ROW_CARRY)
        with pytest.raises(RuntimeError, match=r"\(-6\).*MPC_ENV_CTRL_CARRY"):
            be.lqr_step(z0, C, c, F, None, zs, u, StepOptions(true_dynamics=env), impl=_native.IMPL_WAVE1)
        with pytest.raises(RuntimeError, match=r"\(-1\).*max_linesearch_iter <= 16"):
            be.lqr_step(z0, C, c, F, None, zs, u, StepOptions(true_dynamics=env, max_linesearch_iter=17), impl=ROW_CARRY)


def _no_module_rollout(*a, **k):
    raise AssertionError("a slew-rate solve through a shipped simulator called the module from Python")


def env_solve(z, kind, dtype, flag, tag="a"):
    ns, nc, T, B, lqr_iter = (int(v) for v in z["meta"])
    dx = make_sim(kind, dtype)
    t = lambda k: torch.from_numpy(z[k]).to(dtype).to(DEV)
    prev = torch.full((1, nc), float(z["prev_" + tag][0]), dtype=dtype, device=DEV) if bool(z["has_prev_" + tag][0]) else None
    ctrl = mpc.MPC(ns, nc, T, u_lower=float(z["lower"][0]), u_upper=float(z["upper"][0]), lqr_iter=lqr_iter, verbose=-1,
                   exit_unconverged=False, detach_unconverged=False, linesearch_decay=float(z["decay"][0]),
                   max_linesearch_iter=int(z["max_ls"][0]), grad_method=GradMethods.AUTO_DIFF, eps=float(z["eps"][0]),
                   slew_rate_penalty=float(z["gamma_" + tag][0]), prev_ctrl=prev, row_carry_kernel=flag)
    with torch.no_grad():
        return ctrl(t("x_init"), QuadCost(t("Q"), t("p")), dx)


@pytest.mark.parametrize("kind", ["pendulum", "cartpole"])
def test_whole_slew_solve_on_the_row_carry_kernel(be, monkeypatch, kind):
    """The fixtures mpc_slew_*_f64 (tag a) in float32: with the flag the plans are bound with impl 10 and the solve stays on the device;
    costs within rtol 1e-3 of the flag-off float32 solve, trajectories within 2 d0 + 1e-4 of the float64 fixture (d0: the flag-off
    float32 solve's distance).  In float64 the flag changes nothing, bit for bit."""
    monkeypatch.setattr(lqr_step, "_module_rollout", _no_module_rollout)
    z = golden("mpc_slew_%s_f64" % kind)
    impls = []
    orig = _native.HipBackend.plan_step

    def spy(self, *a, **k):
        impls.append(k.get("impl", 0))
        return orig(self, *a, **k)
    monkeypatch.setattr(_native.HipBackend, "plan_step", spy)
    x_off, u_off, c_off = env_solve(z, kind, torch.float32, False)
    assert impls and all(i == 0 for i in impls), impls
    del impls[:]
    x_on, u_on, c_on = env_solve(z, kind, torch.float32, True)
    assert impls and all(i == ROW_CARRY for i in impls), impls
    assert x_on.is_cuda and x_on.shape == z["x_a"].shape
    d0x, d0u = np.abs(host(x_off) - z["x_a"]).max(), np.abs(host(u_off) - z["u_a"]).max()
    d1x, d1u = np.abs(host(x_on) - z["x_a"]).max(), np.abs(host(u_on) - z["u_a"]).max()
    print(kind, "flag off: d0 x %.3e u %.3e" % (d0x, d0u), "| flag on: x %.3e u %.3e" % (d1x, d1u),
          "| max rel cost on / off %.3e" % np.abs(host(c_on) / host(c_off) - 1).max())
    np.testing.assert_allclose(host(c_on), host(c_off), rtol=1e-3)
    assert d1x <= 2 * d0x + 1e-4, (d1x, d0x)
    assert d1u <= 2 * d0u + 1e-4, (d1u, d0u)
    del impls[:]
    a = env_solve(z, kind, torch.float64, True)
    b = env_solve(z, kind, torch.float64, False)
    assert impls and all(i == 0 for i in impls), impls
    for s, t in zip(a, b):
        assert torch.equal(s, t)
