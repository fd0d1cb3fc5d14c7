"""CPU-only: a slew-rate penalty around an NNDynamics on the pre-bound network loop (`mpc.MPC(planned_network_slew=True)`):
the argument checks of mpc_mlp_linearize_carry (every case returns before a launch), the bindings, the predicate
`MPC._slew_plan`, and the host loop `_iterate_slew` -> `_iterate_network` on a stand-in backend against the reference's
fixtures mpc_slew_nn_f64 / mpc_slew_nn_prev_f64 (float64, the tolerances tests/test_host_logic.py holds them to)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from mpc import _native, mpc
from mpc.dynamics import NNDynamics
from mpc.mpc import GradMethods, QuadCost
from oracle import env_oracle as E
from oracle import lqr_oracle as O
from oracle_backend import OracleBackend, _bound, _np


# ---------------------------------------------------------------------------------------------
# (a) the C entry without a device
# ---------------------------------------------------------------------------------------------
def _net(ns, nc, hidden=100):
    e = _native.MlpDynamics()
    e.n_layers, e.activation, e.passthrough = 2, 0, 1
    e.widths[0], e.widths[1], e.widths[2] = ns + nc, hidden, ns
    for l in range(2):
        e.W[l], e.b[l] = 16, 16
    return e


def test_linearize_carry_argument_checks():
    L = _native.load()
    e = _net(12, 4)
    call = lambda e, ns, nc, N, z=16, ws=16, nbytes=1 << 20: L.mpc_mlp_linearize_carry(
        ctypes.byref(e), ns, nc, N, z, 16, 16, 16, ws, nbytes, None)
    assert call(e, 12, 4, 0) == 0                                       # N = 0: nothing to do
    assert call(e, 12, 4, 8, z=None) == -2                              # MPC_E_NULL
    e.ctrl_carry = 4
    assert call(e, 12, 4, 8) == -5                                      # MPC_E_ARG: the entry takes the network itself
    assert b"ctrl_carry" in L.mpc_lqr_last_error()
    assert call(_net(29, 4), 29, 4, 8) == -1                            # MPC_E_DIMS: the augmented state has 33 entries
    assert b"n_state + n_ctrl <= 32" in L.mpc_lqr_last_error()
    assert call(_net(12, 4), 12, 4, 8, ws=None, nbytes=0) == -5         # no workspace
    assert b"workspace" in L.mpc_lqr_last_error()
    assert call(_net(28, 4), 28, 4, 8, ws=None, nbytes=0) == -5         # 32 entries pass the shape test, stop at the workspace
    # the dense entry keeps refusing the flag
    assert L.mpc_mlp_linearize(ctypes.byref(e), 12, 4, 8, 16, 16, 16, 16, 16, 1 << 20, None) == -5


# ---------------------------------------------------------------------------------------------
# (b) bindings, constructor, predicate
# ---------------------------------------------------------------------------------------------
def test_augmented_spec_keeps_the_network_it_was_made_from():
    dyn = NNDynamics(5, 2, [8])
    spec = _native.MlpSpec([l.weight for l in dyn.fcs], [l.bias for l in dyn.fcs], "sigmoid", True)
    assert spec.inner is None
    aug = spec.augmented()
    assert aug.inner is spec and aug.ctrl_carry == 2 and (aug.n_state, aug.n_ctrl) == (7, 2)
    assert "mpc_mlp_linearize_carry" in _native.EXPORTS and hasattr(_native.HipBackend, "mlp_linearize_carry")


def test_the_flag_is_a_trailing_keyword_and_off_by_default():
    import inspect
    names = list(inspect.signature(mpc.MPC.__init__).parameters)
    assert names[-2:] == ["weight_grad_kernel", "planned_network_slew"]
    assert mpc.MPC(3, 1, 4).planned_network_slew is False
    assert mpc.MPC(3, 1, 4, planned_network_slew=True).planned_network_slew is True


@pytest.fixture
def any_widths(monkeypatch):
    """MlpSpec.supported refuses a CPU tensor before it looks at the widths: answer for it (tests/test_nn_wide_host.py)."""
    monkeypatch.setattr(_native.MlpSpec, "supported", staticmethod(lambda weights, activation, like, bits=3: True))


def test_slew_plan_takes_a_network_only_with_the_flag_and_inside_the_envelope(any_widths):
    be = OracleBackend()
    T, B = 4, 3

    def plan(ns, nc, act="sigmoid", cost=None, x0=None, **kw):
        kw.setdefault("planned_network_slew", True)
        kw.setdefault("grad_method", GradMethods.ANALYTIC)
        ctrl = mpc.MPC(ns, nc, kw.pop("T", T), slew_rate_penalty=0.5, **kw)
        n = ns + nc
        cost = QuadCost(torch.eye(n).expand(T, B, n, n), torch.zeros(T, B, n)) if cost is None else cost
        return ctrl._slew_plan(cost, NNDynamics(ns, nc, [8], activation=act), be, torch.zeros(B, ns) if x0 is None else x0)
    for ns, nc in ((12, 4), (28, 4)):
        spec = plan(ns, nc)
        assert isinstance(spec, _native.MlpSpec) and spec.ctrl_carry == nc and spec.n_state == ns + nc
        assert spec.inner is not None and spec.inner.ctrl_carry == 0 and spec.inner.n_state == ns
    assert plan(12, 4, act="relu").ctrl_carry == 4
    assert plan(12, 4, planned_network_slew=False) is None
    assert plan(29, 4) is None
    assert plan(12, 4, act="elu") is None
    assert plan(12, 4, grad_method=GradMethods.AUTO_DIFF) is None
    assert plan(12, 4, cost=lambda tau: tau.sum(1)) is None
    assert plan(12, 4, reference_du_norm=True, x0=torch.zeros(2, 12)) is None
    assert plan(12, 4, reference_du_norm=True, x0=torch.zeros(1, 12)) is not None
    assert plan(12, 4, T=1) is None

    class NoPlans:                     # a backend without pre-bound network iterations keeps the general loop
        pass
    ctrl = mpc.MPC(12, 4, T, slew_rate_penalty=0.5, planned_network_slew=True)
    assert ctrl._slew_plan(QuadCost(torch.eye(16).expand(T, B, 16, 16), torch.zeros(T, B, 16)), NNDynamics(12, 4, [8]), NoPlans(),
                           torch.zeros(B, 12)) is None


def test_slew_plan_asks_the_library_about_the_augmented_widths(monkeypatch):
    """`MlpSpec.augmented()` does not ask the LDS budget again; the predicate does, with the augmented weights."""
    asked = []

    def supported(weights, activation, like, bits=3):
        asked.append(([weights[0].shape[1]] + [W.shape[0] for W in weights], bits))
        return weights[0].shape[1] == 16            # the network itself yes, its augmentation (20 inputs) no
    monkeypatch.setattr(_native.MlpSpec, "supported", staticmethod(supported))
    T, B = 4, 3
    ctrl = mpc.MPC(12, 4, T, slew_rate_penalty=0.5, planned_network_slew=True)
    cost = QuadCost(torch.eye(16).expand(T, B, 16, 16), torch.zeros(T, B, 16))
    assert ctrl._slew_plan(cost, NNDynamics(12, 4, [8]), OracleBackend(), torch.zeros(B, 12)) is None
    # the network itself: rollout and linearisation; its augmentation is only ever rolled out: the rollout bit alone
    assert asked == [([16, 8, 12], 3), ([20, 8, 16], 1)]


def test_widths_supported_can_ask_for_the_rollout_kernels_alone():
    W = _native.MlpSpec.widths_supported
    assert not W([40, 1024, 32]) and W([40, 1024, 32], bits=1)          # fits the rollout staging, not the Jacobian's buffers
    assert W([16, 100, 12], bits=1) and not W([49, 100, 33], bits=1)


# ---------------------------------------------------------------------------------------------
# (c) the host loop on a stand-in backend
# ---------------------------------------------------------------------------------------------
class _CarryMlp:
    """z' = (u, net(x, u)) on z = (u_prev, x) for oracle.env_oracle.step: CtrlPassthroughDynamics around the oracle's Mlp."""

    def __init__(self, inner, nc):
        self.inner, self.nc = inner, nc


@contextlib.contextmanager
def _carry_steps():
    orig = E.mlp_step

    def step(z, u, net):
        if isinstance(net, _CarryMlp):
            return np.concatenate((np.asarray(u, dtype=np.float64), orig(np.asarray(z)[:, net.nc:], u, net.inner)), 1)
        return orig(z, u, net)
    E.mlp_step = step
    try:
        yield
    finally:
        E.mlp_step = orig


class CarryOracleBackend(OracleBackend):
    """The oracle stand-in whose network calls understand `ctrl_carry` the way the kernels do: the rollout carries the control,
    the linearisation is the network's own (`net.inner`) inside the augmented layout -- what mpc_mlp_linearize_carry writes."""

    def mlp_traj_cost(self, x_init, u, net, C=None, c=None):
        if not net.ctrl_carry:
            return super().mlp_traj_cost(x_init, u, net, C, c)
        assert C is None
        self.calls.append("mlp_traj_cost:carry")
        with _carry_steps():
            x = E.traj(E.MLP, _np(x_init).astype(np.float64), _np(u).astype(np.float64), _CarryMlp(self._mlp(net.inner), net.ctrl_carry))
        return self._t(x, u), None

    def plan_network_iteration(self, x_init, C, c, net, opts, nominals, scratch=None):
        if not net.ctrl_carry:
            return super().plan_network_iteration(x_init, C, c, net, opts, nominals, scratch)
        T, B = C.shape[0], C.shape[1]
        na = x_init.shape[1]
        nc = C.shape[2] - na
        ns = na - nc
        assert net.ctrl_carry == nc and net.inner.n_state == ns
        inner = self._mlp(net.inner)
        carry = _CarryMlp(inner, nc)
        outs = tuple(dict(new_x=nominals[1 - j][0], new_u=nominals[1 - j][1]) for j in (0, 1))
        vouched = []

        def run(j, stream=None):
            self.calls.append("network_iteration:carry")
            cz, cu = (_np(t).astype(np.float64) for t in nominals[j])
            N = (T - 1) * B
            Fl, fl = E.linearize(E.MLP, cz[:-1, :, nc:].reshape(N, ns), cu[:-1].reshape(N, nc), inner)
            aF, af = np.zeros((N, na, na + nc)), np.zeros((N, na))
            aF[:, np.arange(nc), na + np.arange(nc)] = 1.0
            aF[:, nc:, nc:], af[:, nc:] = Fl, fl
            o = O.lqr_step(_np(x_init), _np(C), _np(c), aF.reshape(T - 1, B, na, na + nc), af.reshape(T - 1, B, na), cz, cu,
                           _bound(opts.u_lower), _bound(opts.u_upper), _np(opts.u_zero_I), opts.delta_u, opts.linesearch_decay,
                           opts.max_linesearch_iter, lockstep=self.lockstep, return_gains=True)
            with _carry_steps():
                nx, nu, cs, full, al, _tr, old = E.rollout_batched(
                    E.MLP, carry, _np(x_init).astype(np.float64), _np(C).astype(np.float64), _np(c).astype(np.float64), o["K"], o["k"],
                    cz, cu, _bound(opts.u_lower), _bound(opts.u_upper), opts.linesearch_decay, opts.max_linesearch_iter,
                    delta_u=opts.delta_u, u_zero_I=_np(opts.u_zero_I))
            r = outs[j]
            r["new_x"].copy_(self._t(nx, C)); r["new_u"].copy_(self._t(nu, C))
            r.update(costs=self._t(cs, C), old_costs=self._t(old, C), full_du_norm=self._t(full, C), alpha_du_norm=self._t(full, C),
                     alphas=self._t(al, C), qp_iters=torch.full((B,), int(o["n_qp_iter"]), dtype=torch.int32),
                     status=torch.full((B,), 0 if vouched else 32, dtype=torch.int32))
            return r
        return run, outs, lambda: vouched.append(True)


def _fixture_solve(z, flag):
    ns, nc, T, B = (int(v) for v in z["meta"])
    tt = lambda k: torch.from_numpy(z[k])
    dyn = NNDynamics(ns, nc, [10, 10], activation="sigmoid").double()
    with torch.no_grad():
        for i, fc in enumerate(dyn.fcs):
            fc.weight.copy_(tt("W%d" % i))
            fc.bias.copy_(tt("b%d" % i))
    ctrl = mpc.MPC(ns, nc, T, tt("lo"), tt("hi"), None, lqr_iter=40, verbose=-1, max_linesearch_iter=1,
                   grad_method=GradMethods.ANALYTIC, slew_rate_penalty=float(z["gamma"][0]),
                   prev_ctrl=tt("prev_ctrl") if "prev_ctrl" in z else None, exit_unconverged=False, planned_network_slew=flag)
    with torch.no_grad():
        return ctrl(tt("x_init"), QuadCost(tt("C"), tt("c")), dyn)


@pytest.mark.parametrize("name", ["mpc_slew_nn_f64", "mpc_slew_nn_prev_f64"])
@pytest.mark.parametrize("lockstep", [True, False])
def test_planned_network_slew_solve_matches_the_reference(name, lockstep, any_widths, monkeypatch):
    """The reference's own slew-rate solves around an NNDynamics (tests/test_mpc.py:652-744) through `_iterate_slew` ->
    `_iterate_network` on the augmented problem, float64: (x, u, costs) at the tolerances
    test_host_logic.py::test_slew_rate_penalty_matches_reference holds the general loop to, nothing re-packed per iteration."""
    be = CarryOracleBackend(lockstep=lockstep)
    prev = _native.set_backend_for_testing(be)
    repacked = []
    orig = mpc.MPC._solve_slew_subproblem
    monkeypatch.setattr(mpc.MPC, "_solve_slew_subproblem", lambda self, *a, **k: (repacked.append(1), orig(self, *a, **k))[1])
    try:
        z = golden(name)
        x, u, costs = _fixture_solve(z, True)
        assert not repacked and be.calls.count("network_iteration:carry") >= 2 and "mlp_traj_cost:carry" in be.calls
    finally:
        _native.set_backend_for_testing(prev)
    tol = 1e-9 if lockstep else 2e-4
    assert x.shape == z["x"].shape
    np.testing.assert_allclose(u.numpy(), z["u"], rtol=tol, atol=tol)
    np.testing.assert_allclose(x.numpy(), z["x"], rtol=tol, atol=tol)
    np.testing.assert_allclose(costs.numpy(), z["costs"], rtol=max(tol, 1e-6))
