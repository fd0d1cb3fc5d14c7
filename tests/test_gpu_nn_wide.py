"""GPU parity (-m gpu) of the NNDynamics kernels from 17 to 32 states (csrc/nn_dynamics.hip: nn_wide_rollout_kernel,
nn_wide_linearize_kernel -- the output layer and the state as TWO 16-row accumulator tiles).

The checks are the ones tests/test_gpu_nn.py applies up to 16 states, called here with wide shapes: the same input
recipes, the same float64 oracle (oracle/env_oracle.py, pinned on the reference's own NNDynamics), the same tolerances
(float32 kernels against float64: rtol 1e-3 / atol 1e-4 on x and u, 1e-3 on costs; 2e-3 / 5e-3 / 5e-3 on a whole solve).
The fixture nn_wide_f64 (24 states, 6 controls) is the unmodified reference's output (tests/golden/make_golden_nn_wide.py).

The batched cases were looked at on the CPU before they were fixed here (docs/history/r07.md): the oracle's rollouts are
finite, and no problem's accept / reject margin |J(trial) - J(nominal)| is below 1e-4 (1 + |J(nominal)|) at a trial it runs
-- float32 cannot flip a line-search decision there, the cap on ties in strict_step_check is not what passes them."""
import numpy as np
import pytest
import torch

import test_gpu_nn as base
from test_gpu_fullsize import host

pytestmark = pytest.mark.gpu
DEV = base.DEV
f32 = base.f32


@pytest.fixture(scope="module")
def be():
    from mpc import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()            # fail loudly if the extension is missing
    return _native.HipBackend()


def test_wide_network_kernels_on_the_reference_fixture(be):
    """Forward map and Jacobian at the random points, the nominal trajectory, F and f along it, the line-searched rollout of
    one LQR step and the trajectory cost -- against the reference's own outputs at 24 states / 6 controls."""
    base.test_network_kernels_on_the_reference_fixtures(be, "nn_wide_f64")


@pytest.mark.parametrize("ns,nc,hidden,act,passthrough,B,T,bound", [
    (32, 8, [100], "sigmoid", True, 1024, 64, 0.5),          # BASELINE configuration 5's shape, the reference's default network
    (20, 5, [64, 48], "relu", True, 333, 25, None),          # ragged last group, two hidden layers, unbounded
    (24, 8, [256, 32, 20], "elu", False, 260, 12, 1.0),      # three hidden layers, no passthrough: the second tile half full
    (17, 3, [], "sigmoid", True, 100, 6, None),              # a single Linear layer, ONE row in the second tile
    (28, 4, [100], "sigmoid", True, 300, 20, 1.0),           # the widest network a slew-rate solve augments to 32
])
def test_wide_network_rollout_and_linearisation_at_full_batches(be, ns, nc, hidden, act, passthrough, B, T, bound):
    """Random networks, every problem: nominal trajectory and cost, F / f at all (T-1) B points, the line-searched rollout."""
    base.test_network_rollout_and_linearisation_at_full_batches(be, ns, nc, hidden, act, passthrough, B, T, bound)


def test_wide_network_line_search_runs_every_depth_like_the_reference(be):
    """Costs that are not convex in the state: the sixteen problems of a wavefront stop at every depth of the search."""
    base.test_network_line_search_runs_every_depth_like_the_reference(be, 24, 6, [64], 333, 12, 10, 0.5, 8.0)


def test_wide_network_rollout_with_tensor_bounds_delta_u_and_pinned_controls(be):
    base.test_network_rollout_with_tensor_bounds_delta_u_and_pinned_controls(be, 24, 6, [64])


@pytest.mark.parametrize("ns,nc,hidden", [(20, 4, [32]), (13, 4, [24, 16]), (24, 8, [40])])
def test_wide_ctrl_carry_rollout_matches_the_augmented_map(be, ns, nc, hidden):
    """`MlpSpec.augmented()` with an augmented state of 24, 17 and 32 entries: the carried controls sit in the first tile,
    the network's own outputs straddle both."""
    base.test_ctrl_carry_rollout_matches_the_augmented_map(be, ns, nc, hidden)


def test_mpc_forward_with_a_wide_nndynamics_matches_the_reference_solve(be, monkeypatch):
    """mpc.MPC(...)(x_init, QuadCost, NNDynamics(24, 6, [48])): the iterations run as pre-bound kernel calls (at least two of
    them), and the solve agrees with the reference's float64 one and with this package's host-driven path."""
    base.test_mpc_forward_with_nndynamics_matches_the_reference_solve(be, "nn_wide_f64", monkeypatch)


def test_slew_rate_penalty_on_a_wide_network(be, monkeypatch):
    """slew_rate_penalty around NNDynamics(20, 4, [32]): the augmented state (previous control, x) has 24 entries, so
    CtrlPassthroughDynamics(NNDynamics) rolls out in the two-tile kernel (`ctrl_carry`); against this package's host-driven
    float32 path (the module called timestep by timestep) at the tolerances of the whole-solve checks."""
    from mpc import _native, mpc
    from mpc.dynamics import NNDynamics
    ns, nc, T, B = 20, 4, 8, 12
    torch.manual_seed(11)
    dyn = NNDynamics(ns, nc, [32], activation="sigmoid").to(DEV)
    g = torch.Generator().manual_seed(12)
    n = ns + nc
    A = torch.randn(T, B, n, n, generator=g)
    C = (A.transpose(2, 3) @ A / n + torch.eye(n)).to(DEV)       # (well conditioned: two float32 paths, ten iterations apart)
    c = torch.randn(T, B, n, generator=g).to(DEV)
    x0 = torch.randn(B, ns, generator=g).to(DEV)
    lo = (-0.5 - 0.5 * torch.rand(T, B, nc, generator=g)).to(DEV)
    hi = (0.5 + 0.5 * torch.rand(T, B, nc, generator=g)).to(DEV)
    prev = (0.2 * torch.randn(B, nc, generator=g)).to(DEV)
    carried = []
    orig = _native.HipBackend.mlp_rollout

    def spy(self, *a, **k):
        carried.append((a[9].ctrl_carry, a[9].n_state))
        return orig(self, *a, **k)
    monkeypatch.setattr(_native.HipBackend, "mlp_rollout", spy)

    def solve():
        ctrl = mpc.MPC(ns, nc, T, lo, hi, None, lqr_iter=10, verbose=-1, max_linesearch_iter=1,
                       grad_method=mpc.GradMethods.ANALYTIC, slew_rate_penalty=0.7, prev_ctrl=prev,
                       exit_unconverged=False, backprop=False)
        with torch.no_grad():
            return ctrl(x0, mpc.QuadCost(C, c), dyn)
    x, u, costs = solve()
    torch.cuda.synchronize()
    assert carried and all(cc == (nc, ns + nc) for cc in carried)          # the augmented network ran in the kernel
    n_kernel = len(carried)
    monkeypatch.setattr(NNDynamics, "native_net", lambda self, like: None)
    x2, u2, costs2 = solve()
    assert len(carried) == n_kernel                                         # ... and the second solve did not
    print("slew 20/4: max |du| %.3e, max |dx| %.3e, max rel dcost %.3e" % (
        float((u - u2).abs().max()), float((x - x2).abs().max()), float(((costs - costs2).abs() / costs2.abs()).max())))
    assert torch.isfinite(costs).all() and (host(u) >= host(lo) - 1e-6).all() and (host(u) <= host(hi) + 1e-6).all()
    np.testing.assert_allclose(host(costs), host(costs2), rtol=2e-3)
    np.testing.assert_allclose(host(u), host(u2), rtol=5e-3, atol=5e-3)
    np.testing.assert_allclose(host(x), host(x2), rtol=5e-3, atol=5e-3)
