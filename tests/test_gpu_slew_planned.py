"""GPU tests (-m gpu) of the device-side slew-rate loop (round 11): mpc_slew_augment against the torch composition, the control
carry of the shipped simulators in mpc_env_traj_cost and in the lane-per-problem step (MPC_ENV_CTRL_CARRY), whole solves
against the reference-made fixtures and against the route-off solve, and gradients through the unchanged differentiable ending.

Tolerances: float64 1e-9 (trajectories through a simulator alone: 1e-12); float32 the project's rtol 1e-3 / atol 1e-4; whole
solves against the reference what tests/test_gpu_parity.py applies to ilqr_*_f64 (costs 1e-5, x / u 1e-4) and to the slew
fixtures (2e-4)."""
import numpy as np
import pytest
import torch

from conftest import golden
from mpc import _native, lqr_step, mpc, util
from mpc._native import StepOptions
from mpc.dynamics import CtrlPassthroughDynamics
from mpc.env_dx import cartpole, pendulum
from mpc.mpc import GradMethods, LinDx, QuadCost

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = dict(rtol=1e-3, atol=1e-4)


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()
    return _native.HipBackend()


def host(t):
    return t.detach().cpu().numpy()


def make_sim(kind, dtype=torch.float64):
    dx = {"pendulum": pendulum.PendulumDx, "pendulum_full": lambda: pendulum.PendulumDx(simple=False),
          "cartpole": cartpole.CartpoleDx}[kind]()
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


def route_off(ctrl):
    ctrl._slew_plan = lambda *a, **k: None
    return ctrl


# ---------------------------------------------------------------------------------------------
# (d) mpc_slew_augment == the torch composition, bitwise
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,nc", [(3, 2), (5, 1), (12, 4)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("layout", ["full", "shared", "per_t"])
@pytest.mark.parametrize("with_f", [True, False])
def test_slew_augment_is_the_torch_composition_bitwise(be, ns, nc, dtype, layout, with_f):
    T, B, n, gamma = 3, 5, ns + nc, 0.7
    g = torch.Generator().manual_seed(100 * ns + nc)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    ctrl = mpc.MPC(ns, nc, T, slew_rate_penalty=gamma)
    lead = {"full": (T, B), "shared": (), "per_t": (T,)}[layout]
    cost = ctrl._expand_cost(QuadCost(r(*lead, n, n), r(*lead, n)), B)
    F = r(T - 1, B, ns, n) if layout == "full" else r(ns, n).expand(T - 1, B, ns, n)
    f = (r(T - 1, B, ns) if layout != "shared" else r(ns).expand(T - 1, B, ns)) if with_f else None
    _, wC, wc, wF, wf = ctrl._slew_compose(cost.C, cost.c, F, f)
    aC, ac, aF, af = be.slew_augment(cost.C, cost.c, F, f, ns, nc, gamma, prefill=float("nan"))
    torch.cuda.synchronize()
    for got, want in ((aC, wC), (ac, wc), (aF, wF)):
        assert got.shape == want.shape and got.dtype == dtype
        assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))     # bitwise
    assert (af is None) == (wf is None)
    if with_f:
        assert torch.equal(af, wf)
    if layout == "shared":      # one shared [na,na] block, expanded: stride 0 on both broadcast axes
        assert aC.stride()[:2] == (0, 0) and ac.stride()[:2] == (0, 0) and aF.stride()[:2] == (0, 0)
        assert not with_f or af.stride()[:2] == (0, 0)
    elif layout == "per_t":     # [T,1,na,na]
        assert aC.stride(1) == 0 and ac.stride(1) == 0 and aC.stride(0) != 0
        assert aF.stride()[:2] == (0, 0)
    else:
        assert aC.is_contiguous() and aF.is_contiguous()


def test_slew_augment_without_dynamics_and_empty_batch(be):
    """F None (a simulator carried by the kernels): the cost alone.  B = 0 is a no-op."""
    ns, nc, T, B = 3, 1, 4, 6
    g = torch.Generator().manual_seed(3)
    C = torch.randn(T, B, 4, 4, generator=g, dtype=torch.float64).to(DEV)
    c = torch.randn(T, B, 4, generator=g, dtype=torch.float64).to(DEV)
    ctrl = mpc.MPC(ns, nc, T, slew_rate_penalty=2.0)
    _, wC, wc, _, _ = ctrl._slew_compose(C, c, None, None)
    aC, ac, aF, af = be.slew_augment(C, c, None, None, ns, nc, 2.0, prefill=float("nan"))
    assert aF is None and af is None and torch.equal(aC, wC) and torch.equal(ac, wc)
    out = be.slew_augment(C[:, :0], c[:, :0], None, None, ns, nc, 2.0)
    assert out[0].shape == (T, 0, 5, 5)


# ---------------------------------------------------------------------------------------------
# (e) mpc_env_traj_cost with the carry == the module rollout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pendulum", "pendulum_full", "cartpole"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_env_traj_with_carry_is_the_module_rollout(be, kind, dtype):
    dx = make_sim(kind)
    T, B = 8, 37
    g = torch.Generator().manual_seed(17)
    x0 = sim_states(dx, B, 4).to(dtype).double()
    u = (0.7 * dx._u_max * torch.randn(T, B, 1, generator=g, dtype=torch.float64)).to(dtype).double()     # some beyond the clamp
    prev = torch.randn(B, 1, generator=g, dtype=torch.float64).to(dtype).double()
    assert int((u.abs() > dx._u_max).sum()) >= 5
    mod = CtrlPassthroughDynamics(dx)
    zs = [torch.cat((prev, x0), 1)]
    for t in range(T - 1):
        zs.append(mod(zs[-1], u[t]))
    want = torch.stack(zs).numpy()
    env = make_sim(kind, dtype).native_env().augmented()
    got, cost = be.env_traj_cost(zs[0].to(dtype).to(DEV), u.to(dtype).to(DEV), env)
    torch.cuda.synchronize()
    assert cost is None and got.shape == (T, B, dx.n_state + 1)
    tol = dict(rtol=1e-12, atol=1e-12) if dtype == torch.float64 else F32
    np.testing.assert_allclose(host(got), want, **tol)
    assert torch.equal(got[1:, :, 0], u.to(dtype).to(DEV)[:-1, :, 0])             # carried raw
    # ... and with the cost (the workgroup-per-problem kernel carries the control, too)
    n = dx.n_state + 2
    L = torch.randn(T, B, n, n, generator=g, dtype=torch.float64)
    C, c = (L @ L.transpose(2, 3)).to(dtype).to(DEV), torch.randn(T, B, n, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    got2, cost2 = be.env_traj_cost(zs[0].to(dtype).to(DEV), u.to(dtype).to(DEV), env, C=C, c=c)
    torch.cuda.synchronize()
    np.testing.assert_allclose(host(got2), want, **tol)
    tau = torch.cat((torch.stack(zs), u), 2)
    wcost = (0.5 * torch.einsum("tbi,tbij,tbj->b", tau, C.cpu().double(), tau) + (tau * c.cpu().double()).sum((0, 2))).numpy()
    np.testing.assert_allclose(host(cost2), wcost, rtol=1e-11 if dtype == torch.float64 else 1e-3)


# ---------------------------------------------------------------------------------------------
# (f) one step: the lane-per-problem kernel with carry + linearize == the route-off step on the same nominal
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pendulum", "cartpole"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("max_ls", [1, 3, 10])
def test_carry_step_equals_the_route_off_step(be, monkeypatch, kind, dtype, max_ls):
    dx = make_sim(kind, dtype)
    T, B, ns = 8, 37, dx.n_state
    bound, gamma = (0.6, 0.5) if kind == "pendulum" else (1.5, 0.1)
    g = torch.Generator().manual_seed(23 + max_ls)
    x0 = sim_states(dx, B, 9).to(dtype).to(DEV)
    u = (0.8 * bound * (2 * torch.rand(T, B, 1, generator=g, dtype=torch.float64) - 1)).to(dtype).to(DEV)
    prev = (0.3 * torch.randn(B, 1, generator=g, dtype=torch.float64)).to(dtype).to(DEV)
    q, p = dx.get_true_obj()
    Q = torch.diag(q.to(dtype)).expand(T, B, ns + 1, ns + 1).contiguous().to(DEV)
    pp = p.to(dtype).expand(T, B, ns + 1).contiguous().to(DEV)
    cost = QuadCost(Q, pp)
    ctrl = route_off(mpc.MPC(ns, 1, T, u_lower=-bound, u_upper=bound, verbose=-1, linesearch_decay=dx.linesearch_decay,
                             max_linesearch_iter=max_ls, grad_method=GradMethods.AUTO_DIFF, slew_rate_penalty=gamma, prev_ctrl=prev))
    x = util.get_traj(T, u, x_init=x0, dynamics=dx)
    F, f = ctrl.linearize_dynamics(x, u, dx, diff=False)
    seen = {}
    orig = lqr_step._module_rollout

    def spy(*a, **k):
        out = orig(*a, **k)
        seen["alphas"] = out[5].reshape(-1).clone()
        return out
    monkeypatch.setattr(lqr_step, "_module_rollout", spy)
    with torch.no_grad():
        xo, uo, _, co, fdn, _ = ctrl.solve_lqr_subproblem(x0, Q, pp, F, f, cost, dx, x, u)
    # the new way: the augmented cost once, the simulator behind the carry, linearised inside the kernel
    env = dx.native_env().augmented()
    env.linearize = True
    aC, ac, _, _ = be.slew_augment(Q, pp, None, None, ns, 1, gamma)
    ax = torch.cat((torch.cat((prev.unsqueeze(0), u[:-1])), x), 2)
    r = be.lqr_step(ax[0].contiguous(), aC, ac, None, None, ax, u,
                    StepOptions(u_lower=-bound, u_upper=bound, linesearch_decay=dx.linesearch_decay, max_linesearch_iter=max_ls,
                                true_dynamics=env), impl=_native.IMPL_TINY)
    r0 = be.lqr_step(ax[0].contiguous(), aC, ac, None, None, ax, u,
                     StepOptions(u_lower=-bound, u_upper=bound, linesearch_decay=dx.linesearch_decay, max_linesearch_iter=max_ls,
                                 true_dynamics=env), impl=_native.IMPL_AUTO)
    torch.cuda.synchronize()
    print(kind, dtype, max_ls, "alphas", sorted(set(host(r["alphas"]).round(6).tolist())), "max |du|", float((r["new_u"] - uo).abs().max()),
          "max |dx|", float((r["new_x"][:, :, 1:] - xo).abs().max()), "on a bound", int((r["new_u"].abs() == bound).sum()))
    assert torch.equal(r["new_u"], r0["new_u"]) and torch.equal(r["new_x"], r0["new_x"]), "auto routes the carry to impl 4"
    assert int((r["new_u"].abs() == bound).sum()) > 0, "bounds tight enough that some controls clamp"
    assert torch.equal(r["alphas"], seen["alphas"]), "step sizes exact"
    tol = dict(rtol=1e-9, atol=1e-9) if dtype == torch.float64 else F32
    np.testing.assert_allclose(host(r["new_u"]), host(uo), **tol)
    np.testing.assert_allclose(host(r["new_x"][:, :, 1:]), host(xo), **tol)
    np.testing.assert_allclose(host(r["costs"]), host(co), rtol=tol["rtol"])
    np.testing.assert_allclose(host(r["full_du_norm"]), host(fdn), **tol)
    assert torch.equal(r["new_x"][1:, :, 0], r["new_u"][:-1, :, 0]) and torch.equal(r["new_x"][0, :, 0], prev[:, 0])


def test_carry_is_refused_by_the_other_kernels_on_the_device(be):
    dx = make_sim("pendulum")
    T, B = 4, 3
    env = dx.native_env().augmented()
    z0 = torch.cat((torch.zeros(B, 1, dtype=torch.float64), sim_states(dx, B, 1)), 1).to(DEV)
    u = torch.zeros(T, B, 1, dtype=torch.float64, device=DEV)
    zs, _ = be.env_traj_cost(z0, u, env)
    C = torch.eye(5, dtype=torch.float64, device=DEV).expand(T, B, 5, 5)
    c = torch.zeros(T, B, 5, dtype=torch.float64, device=DEV)
    F = torch.zeros(T - 1, B, 4, 5, dtype=torch.float64, device=DEV)
    for impl in (_native.IMPL_GENERIC, _native.IMPL_WAVE1):
        with pytest.raises(RuntimeError, match=r"\(-6\).*MPC_ENV_CTRL_CARRY"):
            be.lqr_step(z0, C, c, F, None, zs, u, StepOptions(true_dynamics=env), impl=impl)


# ---------------------------------------------------------------------------------------------
# (g) + (h) whole solves
# ---------------------------------------------------------------------------------------------
def env_solve(z, kind, tag, route=True, params_grad=False):
    ns, nc, T, B, lqr_iter = (int(v) for v in z["meta"])
    dx = make_sim(kind)
    if params_grad:
        dx.params = dx.params.to(DEV).requires_grad_(True)
    t = lambda k: torch.from_numpy(z[k]).to(DEV)
    prev = torch.full((1, nc), float(z["prev_" + tag][0]), dtype=torch.float64, device=DEV) if bool(z["has_prev_" + tag][0]) else None
    ctrl = mpc.MPC(ns, nc, T, u_lower=float(z["lower"][0]), u_upper=float(z["upper"][0]), lqr_iter=lqr_iter, verbose=-1,
                   exit_unconverged=False, detach_unconverged=False, linesearch_decay=float(z["decay"][0]),
                   max_linesearch_iter=int(z["max_ls"][0]), grad_method=GradMethods.AUTO_DIFF, eps=float(z["eps"][0]),
                   slew_rate_penalty=float(z["gamma_" + tag][0]), prev_ctrl=prev)
    if not route:
        route_off(ctrl)
    return ctrl(t("x_init"), QuadCost(t("Q"), t("p")), dx), dx


def _no_module_rollout(*a, **k):
    raise AssertionError("a slew-rate solve through a shipped simulator called the module from Python")


@pytest.mark.parametrize("kind", ["pendulum", "cartpole"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_simulator_slew_solve_stays_on_the_device_and_matches_the_reference(be, monkeypatch, kind, tag):
    """(h) part one, the test that fails without the route: with the per-timestep module rollout forbidden, a PendulumDx and a
    CartpoleDx slew solve complete -- and (g) equal the reference's (a: gamma = 0.5, b: gamma = 2 with prev_ctrl = 0.3) at the
    tolerances of test_gpu_parity's ilqr_*_f64 cases.  Every problem is held to them: none is excused as a tie."""
    monkeypatch.setattr(lqr_step, "_module_rollout", _no_module_rollout)
    z = golden("mpc_slew_%s_f64" % kind)
    with torch.no_grad():
        (x, u, costs), _ = env_solve(z, kind, tag)
    assert x.is_cuda and x.shape == z["x_" + tag].shape
    print(kind, tag, "max |du|", np.abs(host(u) - z["u_" + tag]).max(), "max |dx|", np.abs(host(x) - z["x_" + tag]).max(),
          "max rel cost", np.abs(host(costs) / z["costs_" + tag] - 1).max())
    np.testing.assert_allclose(host(costs), z["costs_" + tag], rtol=1e-5)
    np.testing.assert_allclose(host(x), z["x_" + tag], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(host(u), z["u_" + tag], rtol=1e-4, atol=1e-4)
    if kind == "pendulum" and tag == "a":
        assert int((np.abs(z["u_a"]) == float(z["upper"][0])).sum()) >= 4, "this fixture keeps the box QP exercised"


def lin_solve(z, route, grad=False):
    ns, nc, T, B, lqr_iter = (int(v) for v in z["meta"])
    t = {k: torch.from_numpy(z[k]).to(DEV) for k in ("x_init", "C", "c", "F", "f")}
    if grad:
        for k in ("x_init", "C", "c"):
            t[k].requires_grad_(True)
    ctrl = mpc.MPC(ns, nc, T, u_lower=-float(z["bound"][0]), u_upper=float(z["bound"][0]), lqr_iter=lqr_iter, verbose=-1,
                   exit_unconverged=False, detach_unconverged=False, slew_rate_penalty=float(z["gamma"][0]))
    if not route:
        route_off(ctrl)
    return ctrl(t["x_init"], QuadCost(t["C"], t["c"]), LinDx(t["F"], t["f"])), t


def test_lindx_slew_solve_repacks_nothing_and_matches_the_reference(be, monkeypatch):
    """(h) part two: a LinDx slew solve without gradients never calls _solve_slew_subproblem; (g) it equals mpc_slew_lin_f64 at
    the 2e-4 of the slew fixtures and the route-off solve at 1e-9."""
    z = golden("mpc_slew_lin_f64")
    calls = []
    orig = mpc.MPC._solve_slew_subproblem
    monkeypatch.setattr(mpc.MPC, "_solve_slew_subproblem", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    with torch.no_grad():
        (x, u, costs), _ = lin_solve(z, True)
        assert not calls
        (xo, uo, co), _ = lin_solve(z, False)
    assert calls
    np.testing.assert_allclose(host(u), z["u"], rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(host(x), z["x"], rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(host(costs), z["costs"], rtol=2e-4)
    np.testing.assert_allclose(host(u), host(uo), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(x), host(xo), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(costs), host(co), rtol=1e-9)


@pytest.mark.parametrize("shared_cost", [False, True])
def test_headline_shape_slew_solve_new_route_against_route_off(be, shared_cost):
    """12/4 -> 16/4, T = 6, B = 9, float32, box-constrained: the planned route (which makes the nominal / symmetry promises to
    the fused kernels) against the route-off solve at the float32 tolerance; also with one shared [n,n] cost (stride 0 kept)."""
    ns, nc, T, B, n = 12, 4, 6, 9, 16
    g = torch.Generator().manual_seed(41)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    L = r(n, n) if shared_cost else r(T, B, n, n)
    C = (L @ L.transpose(-1, -2) + torch.eye(n, dtype=torch.float64)).float().to(DEV)
    c = (r(n) if shared_cost else r(T, B, n)).float().to(DEV)
    F = (0.2 * r(T - 1, B, ns, n) + torch.cat((torch.eye(ns, dtype=torch.float64), torch.zeros(ns, nc, dtype=torch.float64)), 1)).float().to(DEV)
    f = (0.1 * r(T - 1, B, ns)).float().to(DEV)
    x0 = r(B, ns).float().to(DEV)
    prev = (0.2 * r(B, nc)).float().to(DEV)
    outs = []
    for route in (True, False):
        ctrl = mpc.MPC(ns, nc, T, u_lower=-0.3, u_upper=0.3, lqr_iter=5, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                       n_batch=B, slew_rate_penalty=1.0, prev_ctrl=prev)
        if not route:
            route_off(ctrl)
        with torch.no_grad():
            outs.append(ctrl(x0, QuadCost(C, c), LinDx(F, f)))
    (x, u, costs), (xo, uo, co) = outs
    print("shared" if shared_cost else "full", "max |du|", float((u - uo).abs().max()), "max |dx|", float((x - xo).abs().max()),
          "on a bound", int((u.abs() == 0.3).sum()))
    assert int((u.abs() == 0.3).sum()) > 0
    np.testing.assert_allclose(host(u), host(uo), **F32)
    np.testing.assert_allclose(host(x), host(xo), **F32)
    np.testing.assert_allclose(host(costs), host(co), rtol=1e-3)


# ---------------------------------------------------------------------------------------------
# (i) gradients go through unchanged code: new route == route off
# ---------------------------------------------------------------------------------------------
def test_lindx_slew_gradients_equal_route_off(be):
    z = golden("mpc_slew_lin_f64")
    g = torch.Generator().manual_seed(8)
    wx = torch.randn(z["x"].shape, generator=g, dtype=torch.float64).to(DEV)
    wu = torch.randn(z["u"].shape, generator=g, dtype=torch.float64).to(DEV)
    grads = []
    for route in (True, False):
        (x, u, _), t = lin_solve(z, route, grad=True)
        grads.append(torch.autograd.grad((x * wx).sum() + (u * wu).sum(), [t["C"], t["c"], t["x_init"]]))
    for a, b, name in zip(grads[0], grads[1], ("C", "c", "x_init")):
        assert float(b.abs().max()) > 0
        np.testing.assert_allclose(host(a), host(b), rtol=1e-9, atol=1e-9 * float(b.abs().max()), err_msg=name)


@pytest.mark.parametrize("kind", ["pendulum", "cartpole"])
def test_simulator_slew_parameter_gradient_equals_route_off(be, kind):
    z = golden("mpc_slew_%s_f64" % kind)
    g = torch.Generator().manual_seed(9)
    wx = torch.randn(z["x_b"].shape, generator=g, dtype=torch.float64).to(DEV)
    wu = torch.randn(z["u_b"].shape, generator=g, dtype=torch.float64).to(DEV)
    grads = []
    for route in (True, False):
        (x, u, _), dx = env_solve(z, kind, "b", route=route, params_grad=True)
        grads.append(torch.autograd.grad((x * wx).sum() + (u * wu).sum(), [dx.params])[0])
    assert float(grads[1].abs().max()) > 0
    np.testing.assert_allclose(host(grads[0]), host(grads[1]), rtol=1e-9, atol=1e-9 * float(grads[1].abs().max()))
