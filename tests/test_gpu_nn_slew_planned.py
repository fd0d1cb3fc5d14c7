"""GPU (-m gpu): a slew-rate penalty around an NNDynamics on the pre-bound device loop, `mpc.MPC(planned_network_slew=True)`.

(1) mpc_mlp_linearize_carry -- the network's linearisation written straight into the augmented layout (state (u_prev, x),
    aF = [[0 0 I], [0 F]], af = [0; f]) -- bitwise against mpc_mlp_linearize on the sliced points, every constant element exact,
    no element left unwritten (outputs full of NaN beforehand), through the register-resident, the LDS-staged and the two-tile
    kernels; one network of each family against the float64 oracle at the tolerances of tests/test_gpu_nn.py.
(2) whole solves of the reference's fixtures with the flag on: no module rollout, no HipBackend.mlp_rollout, one pre-bound
    plan on the augmented network; at the tolerances tests/test_gpu_nn.py::test_slew_rate_penalty_on_the_network_kernels holds
    the general loop to.
(3) flag on against flag off on random problems.
(4) gradients with the flag on against the fixtures' reference gradients; the scale of each bound is the float32 error of the
    flag-off solve, measured in the same test."""
import numpy as np
import pytest
import torch

import test_gpu_nn as base
from conftest import golden
from test_gpu_fullsize import host

pytestmark = pytest.mark.gpu
DEV = base.DEV
f32 = base.f32

NETS = [
    (12, 4, [100]),          # register-resident kernel (the reference's default network)
    (13, 3, [24]),           # register-resident, n_state not a multiple of 4
    (4, 4, [32]),            # register-resident
    (6, 2, [16, 16]),        # LDS-staged, three layers
    (14, 4, [40]),           # LDS-staged, n_state + n_ctrl > 16
    (5, 2, []),              # a single layer
    (20, 4, [32]),           # two output tiles
    (24, 8, [40]),           # two output tiles, augmented state of 32
]


@pytest.fixture(scope="module")
def be():
    from mpc import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()            # fail loudly if the extension is missing
    return _native.HipBackend()


def _points(ns, nc, N, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(N, nc + ns), 0.5 * rng.randn(N, nc)


def _carry_call(be, sp, z, u):
    N, na = z.shape
    nc = u.shape[1]
    aF = torch.full((N, na, na + nc), float("nan"), device=DEV)
    af = torch.full((N, na), float("nan"), device=DEV)
    be.mlp_linearize_carry(sp, z, u, out_F=aF, out_f=af)
    torch.cuda.synchronize()
    return aF, af


@pytest.mark.parametrize("passthrough", [True, False])
@pytest.mark.parametrize("act", ["sigmoid", "relu", "elu"])
@pytest.mark.parametrize("ns,nc,hidden", NETS)
def test_linearize_carry_is_the_dense_linearisation_in_the_augmented_layout(be, ns, nc, hidden, act, passthrough):
    sp = base.spec_of(base.random_net(ns, nc, hidden, act, passthrough, seed=ns * 10 + nc))
    na = ns + nc
    for N in (1, 37, 49):            # one lane of one wavefront; three wavefronts, the last ragged; a full group more
        zn, un = _points(ns, nc, N, N)
        z, u = f32(zn), f32(un)
        aF, af = _carry_call(be, sp, z, u)
        F, f = be.mlp_linearize(sp, z[:, nc:], u)
        torch.cuda.synchronize()
        assert not torch.isnan(aF).any() and not torch.isnan(af).any(), "an element was left unwritten"
        assert torch.equal(aF[:, nc:, nc:], F) and torch.equal(af[:, nc:], f), "the network block must be bitwise the dense entry's"
        carry = torch.zeros(nc, na + nc, device=DEV)
        carry[torch.arange(nc), na + torch.arange(nc)] = 1.0
        assert torch.equal(aF[:, :nc], carry.expand(N, nc, na + nc))
        assert (aF[:, nc:, :nc] == 0).all() and (af[:, :nc] == 0).all()


@pytest.mark.parametrize("act,passthrough", [("sigmoid", True), ("relu", False)])
@pytest.mark.parametrize("ns,nc,hidden", [(12, 4, [100]), (6, 2, [16, 16]), (20, 4, [32])])
def test_linearize_carry_against_the_float64_oracle(be, ns, nc, hidden, act, passthrough):
    """One network of each kernel family against oracle.env_oracle.linearize (float64), rtol 1e-3 / atol 1e-4 as
    tests/test_gpu_nn.py holds mpc_mlp_linearize to (the bitwise test above compares with the dense entry, which runs the same
    kernels: this one does not)."""
    from oracle import env_oracle as E
    net = base.random_net(ns, nc, hidden, act, passthrough, seed=ns * 10 + nc)
    zn, un = _points(ns, nc, 37, 5)
    zn, un = zn.astype(np.float32).astype(np.float64), un.astype(np.float32).astype(np.float64)
    aF, af = _carry_call(be, base.spec_of(net), f32(zn), f32(un))
    Fo, fo = E.linearize(E.MLP, zn[:, nc:], un, net)
    scale = 1.0 + np.abs(zn).max()
    np.testing.assert_allclose(host(aF)[:, nc:, nc:], Fo, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(host(af)[:, nc:], fo, rtol=1e-3, atol=1e-4 * scale)


def _fixture_module(z):
    from mpc.dynamics import NNDynamics
    ns, nc = (int(v) for v in z["meta"][:2])
    dyn = NNDynamics(ns, nc, [10, 10], activation="sigmoid")
    with torch.no_grad():
        for i, fc in enumerate(dyn.fcs):
            fc.weight.copy_(torch.from_numpy(z["W%d" % i]).float())
            fc.bias.copy_(torch.from_numpy(z["b%d" % i]).float())
    return dyn.to(DEV)


@pytest.mark.parametrize("name", ["mpc_slew_nn_f64", "mpc_slew_nn_prev_f64"])
def test_planned_slew_solve_runs_pre_bound_and_matches_the_reference(be, name, monkeypatch):
    """The fixtures of test_slew_rate_penalty_on_the_network_kernels, its settings and its tolerances, with the flag on:
    the module is never rolled out timestep by timestep, HipBackend.mlp_rollout (the general loop's call) is never made, and
    ONE plan is bound on the augmented network."""
    from mpc import _native, lqr_step, mpc
    z = golden(name)
    ns, nc, T, B = (int(v) for v in z["meta"])
    dyn = _fixture_module(z)

    def refuse(*a, **k):
        raise AssertionError("the planned route must not roll the module out from Python")
    monkeypatch.setattr(lqr_step, "_module_rollout", refuse)
    rollouts, plans = [], []
    orig_roll, orig_plan = _native.HipBackend.mlp_rollout, _native.HipBackend.plan_network_iteration
    monkeypatch.setattr(_native.HipBackend, "mlp_rollout", lambda self, *a, **k: (rollouts.append(1), orig_roll(self, *a, **k))[1])
    monkeypatch.setattr(_native.HipBackend, "plan_network_iteration",
                        lambda self, *a, **k: (plans.append((a[3].ctrl_carry, a[3].inner is not None, a[0].shape[1])),
                                               orig_plan(self, *a, **k))[1])
    prev = f32(z["prev_ctrl"]) if "prev_ctrl" in z else None
    ctrl = mpc.MPC(ns, nc, T, f32(z["lo"]), f32(z["hi"]), None, lqr_iter=40, verbose=-1, max_linesearch_iter=1,
                   grad_method=mpc.GradMethods.ANALYTIC, slew_rate_penalty=float(z["gamma"][0]), prev_ctrl=prev,
                   exit_unconverged=False, backprop=False, planned_network_slew=True)
    with torch.no_grad():
        x, u, costs = ctrl(f32(z["x_init"]), mpc.QuadCost(f32(z["C"]), f32(z["c"])), dyn)
    torch.cuda.synchronize()
    assert not rollouts
    assert plans == [(nc, True, ns + nc)]
    assert x.shape == z["x"].shape
    np.testing.assert_allclose(host(u), z["u"], rtol=5e-3, atol=5e-3)
    np.testing.assert_allclose(host(x), z["x"], rtol=5e-3, atol=5e-3)
    np.testing.assert_allclose(host(costs), z["costs"], rtol=2e-3)


def _random_problem(ns, nc, hidden, T, B, seed):
    from mpc.dynamics import NNDynamics
    torch.manual_seed(seed)
    dyn = NNDynamics(ns, nc, hidden, activation="sigmoid").to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    n = ns + nc
    A = torch.randn(T, B, n, n, generator=g)
    C = (A.transpose(2, 3) @ A / n + torch.eye(n)).to(DEV)       # (well conditioned: two float32 paths, ten iterations apart)
    c = torch.randn(T, B, n, generator=g).to(DEV)
    x0 = torch.randn(B, ns, generator=g).to(DEV)
    return dyn, C, c, x0, g


def _both_routes(ns, nc, T, dyn, C, c, x0, lo, hi, prev, max_ls, monkeypatch):
    from mpc import _native, mpc
    out, planned = [], []
    orig = _native.HipBackend.plan_network_iteration
    monkeypatch.setattr(_native.HipBackend, "plan_network_iteration",
                        lambda self, *a, **k: (planned.append((flag, a[3].ctrl_carry)), orig(self, *a, **k))[1])
    for flag in (True, False):
        ctrl = mpc.MPC(ns, nc, T, lo, hi, None, lqr_iter=10, verbose=-1, max_linesearch_iter=max_ls,
                       grad_method=mpc.GradMethods.ANALYTIC, slew_rate_penalty=0.7, prev_ctrl=prev,
                       exit_unconverged=False, backprop=False, planned_network_slew=flag)
        with torch.no_grad():
            out.append(ctrl(x0, mpc.QuadCost(C, c), dyn))
    torch.cuda.synchronize()
    assert planned == [(True, nc)], "flag on: one pre-bound plan on the augmented network; flag off: the general loop"
    (x, u, costs), (x2, u2, costs2) = out
    print("flag on / off: max |du| %.3e, max |dx| %.3e, max rel dcost %.3e" % (
        float((u - u2).abs().max()), float((x - x2).abs().max()), float(((costs - costs2).abs() / costs2.abs()).max())))
    assert x.shape == x2.shape and torch.isfinite(costs).all()
    return (x, u, costs), (x2, u2, costs2)


def test_flag_on_against_flag_off_on_a_wide_network(be, monkeypatch):
    """The recipe of tests/test_gpu_nn_wide.py::test_slew_rate_penalty_on_a_wide_network (20/4: an augmented state of 24, the
    two-tile kernels, tensor bounds, prev_ctrl)."""
    ns, nc, T, B = 20, 4, 8, 12
    torch.manual_seed(11)
    from mpc.dynamics import NNDynamics
    dyn = NNDynamics(ns, nc, [32], activation="sigmoid").to(DEV)
    g = torch.Generator().manual_seed(12)
    n = ns + nc
    A = torch.randn(T, B, n, n, generator=g)
    C = (A.transpose(2, 3) @ A / n + torch.eye(n)).to(DEV)
    c = torch.randn(T, B, n, generator=g).to(DEV)
    x0 = torch.randn(B, ns, generator=g).to(DEV)
    lo = (-0.5 - 0.5 * torch.rand(T, B, nc, generator=g)).to(DEV)
    hi = (0.5 + 0.5 * torch.rand(T, B, nc, generator=g)).to(DEV)
    prev = (0.2 * torch.randn(B, nc, generator=g)).to(DEV)
    (x, u, costs), (x2, u2, costs2) = _both_routes(ns, nc, T, dyn, C, c, x0, lo, hi, prev, 1, monkeypatch)
    assert (host(u) >= host(lo) - 1e-6).all() and (host(u) <= host(hi) + 1e-6).all()
    np.testing.assert_allclose(host(costs), host(costs2), rtol=2e-3)


@pytest.mark.parametrize("max_ls", [1, 10])
def test_flag_on_against_flag_off_on_the_default_network(be, max_ls, monkeypatch):
    """NNDynamics(12, 4, [100]) -- the register-resident kernels on the network, the staged rollout on its augmentation -- T = 6,
    B = 9, box +-0.3.  Costs only: with a line search, ties in alpha may move single controls between two float32 routes."""
    ns, nc, T, B = 12, 4, 6, 9
    dyn, C, c, x0, g = _random_problem(ns, nc, [100], T, B, 21)
    (x, u, costs), (x2, u2, costs2) = _both_routes(ns, nc, T, dyn, C, c, x0, -0.3, 0.3, None, max_ls, monkeypatch)
    assert float(u.abs().max()) <= 0.3 + 1e-6
    np.testing.assert_allclose(host(costs), host(costs2), rtol=2e-3)


@pytest.mark.parametrize("name", ["mpc_slew_nn_f64", "mpc_slew_nn_prev_f64"])
def test_gradients_with_the_flag_on_against_the_reference(be, name, monkeypatch):
    """The loss of tests/test_host_logic.py::run_slew_golden in float32: gC, gc, gx0, gb0 with the flag on against the
    fixture's reference gradients.  Bound of each: max(2 x the flag-off float32 solve's own deviation from the fixture,
    1e-3 max|g|) -- the yardstick is the reference, the parent route's float32 error sets the scale, and the factor 2 allows
    that two float32 solves land on different sides of the converged answer.
    Measured on one MI355X (max |g - g_ref| flag on / flag off, see docs/history/r12.md)."""
    from mpc import _native, mpc
    z = golden(name)
    ns, nc, T, B = (int(v) for v in z["meta"])
    planned = []
    orig = _native.HipBackend.plan_network_iteration
    monkeypatch.setattr(_native.HipBackend, "plan_network_iteration",
                        lambda self, *a, **k: (planned.append(a[3].ctrl_carry), orig(self, *a, **k))[1])

    def grads(flag):
        dyn = _fixture_module(z)
        C, c, x0 = (f32(z[k]).requires_grad_(True) for k in ("C", "c", "x_init"))
        prev = f32(z["prev_ctrl"]) if "prev_ctrl" in z else None
        ctrl = mpc.MPC(ns, nc, T, f32(z["lo"]), f32(z["hi"]), None, lqr_iter=40, verbose=-1, max_linesearch_iter=1,
                       grad_method=mpc.GradMethods.ANALYTIC, slew_rate_penalty=float(z["gamma"][0]), prev_ctrl=prev,
                       exit_unconverged=False, planned_network_slew=flag)
        x, u, costs = ctrl(x0, mpc.QuadCost(C, c), dyn)
        loss = (x * f32(z["wx"])).sum() + (u * f32(z["wu"])).sum()
        return [host(t).astype(np.float64) for t in torch.autograd.grad(loss, [C, c, x0, dyn.fcs[0].bias])]
    on = grads(True)
    assert planned == [nc], "flag on: the solve in front of the differentiable ending ran pre-bound on the augmented network"
    off = grads(False)
    assert planned == [nc], "flag off: the general loop"
    failed = []
    for key, g_on, g_off in zip(("gC", "gc", "gx0", "gb0"), on, off):
        ref = z[key]
        d_on, d_off = np.abs(g_on - ref).max(), np.abs(g_off - ref).max()
        bound = max(2.0 * d_off, 1e-3 * np.abs(ref).max())
        print("%s %s: max |g - g_ref| flag on %.3e, flag off %.3e, bound %.3e (max |g_ref| %.3e)" % (
            name, key, d_on, d_off, bound, np.abs(ref).max()))
        if not d_on <= bound:
            failed.append(key)
    assert not failed, failed
