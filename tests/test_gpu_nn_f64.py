"""GPU parity (-m gpu) of the float64 NNDynamics kernels (csrc/nn_dynamics64.hip, mpc_mlp_*_dtype with MPC_F64: plain FMA, one
wavefront per problem / point) against oracle/env_oracle.py and the reference's own recorded outputs (tests/golden/nn_*_f64.npz),
and of whole float64 solves on the `network` route against the module path.

The bar is the project's float64 one: |err| <= 1e-9 (1 + max |reference array|) on x, u, F, f, rtol 1e-9 on costs and norms, the
line search's alphas exactly.  (The kernels keep the reference's running product alpha *= decay, mpc/lqr_step.py:247; the
oracle's decay ** i is the same double for the trials these cases reach, i <= 3 -- `running` maps it for any i.)"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-9
NN_CASES = ["nn_sigmoid_f64", "nn_relu2_f64", "nn_headline_f64", "nn_nopass_f64"]


@pytest.fixture(scope="module")
def be():
    from mpc import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()            # fail loudly if the extension is missing
    return _native.HipBackend()


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def spec_of(net):
    from mpc._native import MlpSpec
    return MlpSpec([f64(W) for W in net.Ws], [f64(b) for b in net.bs], net.activation, net.passthrough)


def random_net(ns, nc, hidden, act, passthrough, seed, scale=1.0):
    """tests/test_gpu_nn.py's recipe."""
    from oracle import env_oracle as E
    rng = np.random.RandomState(seed)
    sizes = [ns + nc] + list(hidden) + [ns]
    Ws = [scale * rng.uniform(-1, 1, (o, i)) / np.sqrt(i) for i, o in zip(sizes, sizes[1:])]
    bs = [rng.uniform(-1, 1, o) / np.sqrt(i) for i, o in zip(sizes, sizes[1:])]
    return E.Mlp(Ws, bs, act, passthrough)


def close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    err = np.abs(got - want).max() if want.size else 0.0
    assert err <= BAR * (1.0 + (np.abs(want).max() if want.size else 0.0)), (what, err)


def running(alphas, decay):
    table = np.cumprod(np.concatenate(([1.0], np.full(16, decay))))
    return table[np.rint(np.log(alphas) / np.log(decay)).astype(int)]


def pre_activations(net, x, u):
    """Every hidden layer's pre-activation at the points x [N,ns], u [N,nc] (what a relu / elu kink is measured on)."""
    from oracle import env_oracle as E
    z = np.concatenate((x, u), 1)
    pre = []
    for W, b in zip(net.Ws[:-1], net.bs[:-1]):
        h = z @ W.T + b
        pre.append(h)
        z = E._act(h, net.activation)
    return pre


# ---------------------------------------------------------------------------------------------
# 1. the reference's fixtures
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NN_CASES)
def test_float64_network_kernels_on_the_reference_fixtures(be, name):
    """The sequence of tests/test_gpu_nn.py::test_network_kernels_on_the_reference_fixtures in double, against the REFERENCE's
    own outputs: forward / Jacobian at the random points, the nominal trajectory, F and f along it, the LQR step's line-searched
    rollout (gains from the float64 C oracle's sweep), the trajectory cost."""
    from mpc._native import StepOptions
    from oracle import env_oracle as E
    from oracle import lqr_oracle as O
    z = golden(name)
    ns, nc, T, B = (int(v) for v in z["meta"][:4])
    net = E.Mlp.from_npz(z)
    sp = spec_of(net)
    x1, _ = be.mlp_traj_cost(f64(z["px"]), f64(np.stack((z["pu"], z["pu"]))), sp)
    close(host(x1)[1], z["pnext"], "forward")
    F, f = be.mlp_linearize(sp, f64(z["px"]), f64(z["pu"]))
    close(host(F)[:, :, :ns], z["pR"], "R")
    close(host(F)[:, :, ns:], z["pS"], "S")
    tau = np.concatenate((z["px"], z["pu"]), 1)
    close(host(f), z["pnext"] - np.einsum("nij,nj->ni", np.concatenate((z["pR"], z["pS"]), 2), tau), "f")
    xs, _ = be.mlp_traj_cost(f64(z["x_init"]), f64(z["step_cur_u"]), sp)
    close(host(xs), z["step_cur_x"], "nominal trajectory")
    Fl, fl = be.mlp_linearize(sp, f64(z["step_cur_x"][:-1].reshape(-1, ns)), f64(z["step_cur_u"][:-1].reshape(-1, nc)))
    close(host(Fl).reshape(z["step_F"].shape), z["step_F"], "step_F")
    close(host(fl).reshape(z["step_f"].shape), z["step_f"], "step_f")
    bound = float(z["bound"][0])
    lo, hi = (None, None) if np.isnan(bound) else (-bound, bound)
    decay, max_ls = float(z["decay"][0]), int(z["max_ls"][0])
    o = O.lqr_step(z["x_init"], z["C"], z["c"], z["step_F"], z["step_f"], z["step_cur_x"], z["step_cur_u"], lo, hi,
                   linesearch_decay=decay, max_linesearch_iter=max_ls, return_gains=True)
    old = E.quad_cost(z["C"], z["c"], z["step_cur_x"], z["step_cur_u"])
    r = be.mlp_rollout(f64(z["x_init"]), f64(z["C"]), f64(z["c"]), f64(o["K"]), f64(o["k"]), f64(z["step_cur_x"]),
                       f64(z["step_cur_u"]), f64(old), StepOptions(u_lower=lo, u_upper=hi, linesearch_decay=decay,
                                                                  max_linesearch_iter=max_ls), sp)
    torch.cuda.synchronize()
    close(host(r["new_u"]), z["step_new_u"], "step_new_u")
    close(host(r["new_x"]), z["step_new_x"], "step_new_x")
    np.testing.assert_allclose(host(r["costs"]), z["step_costs"], rtol=BAR)
    # (the fixture's step_full_du_norm is the reference's norm over the transposed array, include/mpc_lqr.h (12): not this output)
    assert (host(r["status"]) == 0).all()
    _, c0 = be.mlp_traj_cost(f64(z["x_init"]), f64(z["step_cur_u"]), sp, C=f64(z["C"]), c=f64(z["c"]))
    np.testing.assert_allclose(host(c0), old, rtol=BAR)


# ---------------------------------------------------------------------------------------------
# 2. random networks: every problem and every point, no exclusions
# ---------------------------------------------------------------------------------------------
RANDOM_CASES = [
    # ns, nc, hidden, act, passthrough, B, T, bound, s, a, must backtrack
    (3, 2, [], "sigmoid", True, 5, 6, None, 3.0, 0.3, False),            # a bare Linear layer
    (12, 4, [100], "sigmoid", True, 67, 9, 0.5, 5.0, 0.2, True),         # the headline network, a ragged batch above 64
    (5, 1, [64, 48], "relu", True, 33, 7, 2.0, 3.0, 0.3, True),          # one control, two hidden layers
    (16, 8, [40, 32, 20], "elu", False, 17, 5, 1.0, 3.0, 0.3, True),     # four layers, no passthrough
    (32, 8, [100], "sigmoid", True, 9, 4, None, 3.0, 0.3, False),        # two state tiles of the float32 kernels
    (17, 3, [24, 24], "relu", True, 19, 6, 0.7, 3.0, 0.3, True),         # odd sizes
    # networks past the 96 KiB a block stages in LDS: the kernels that read the weights in place (IN_PLACE below)
    (12, 4, [128, 128], "relu", True, 9, 5, 0.5, 3.0, 0.3, False),
    (32, 8, [256, 256], "sigmoid", True, 5, 4, None, 3.0, 0.3, False),   # ... and a linearisation area that leaves one wavefront a block
]
IN_PLACE = {(12, 4, 128), (32, 8, 256)}
STAGED_MAX_BYTES = 96 * 1024


def staged_bytes(ns, nc, hidden):
    """Bytes of the network as a block stages it (csrc/nn_dynamics64.h net_layout: rows on an odd stride of doubles, then the biases)."""
    sizes = [ns + nc] + list(hidden) + [ns]
    return 8 * sum(o * (i | 1) + o for i, o in zip(sizes, sizes[1:]))


@pytest.mark.parametrize("ns,nc,hidden,act,passthrough,B,T,bound,s,a,backtracks", RANDOM_CASES)
def test_float64_rollout_and_linearisation_on_random_networks(be, ns, nc, hidden, act, passthrough, B, T, bound, s, a, backtracks):
    from mpc._native import StepOptions
    from oracle import env_oracle as E
    from oracle import lqr_oracle as O
    # both weight paths are run: a row either fits the staging limit or is one of the rows meant to exceed it
    assert (staged_bytes(ns, nc, hidden) > STAGED_MAX_BYTES) == ((ns, nc, (hidden or [0])[0]) in IN_PLACE)
    net = random_net(ns, nc, hidden, act, passthrough, seed=100 * ns + nc, scale=s)
    sp = spec_of(net)
    rng = np.random.RandomState(B)
    n = ns + nc
    x0 = rng.randn(B, ns)
    u0 = 0.3 * rng.randn(T, B, nc)
    if bound is not None:
        u0 = np.clip(u0, -bound, bound)
    A = a * rng.randn(T, B, n, n)
    C = np.einsum("tbki,tbkj->tbij", A, A) + 0.1 * np.eye(n)
    c = rng.randn(T, B, n)
    xs = E.traj(E.MLP, x0, u0, net)
    old = E.quad_cost(C, c, xs, u0)
    Fl, fl = E.linearize(E.MLP, xs[:-1].reshape(-1, ns), u0[:-1].reshape(-1, nc), net)
    lo, hi = (None, None) if bound is None else (-bound, bound)
    decay, max_ls = 0.2, 6
    o = O.lqr_step(x0, C, c, Fl.reshape(T - 1, B, ns, n), fl.reshape(T - 1, B, ns), xs, u0, lo, hi, linesearch_decay=decay,
                   max_linesearch_iter=max_ls, lockstep=False, nthreads=O.max_threads(), return_gains=True)
    nx, nu, costs, full, alphas, trials, old2 = E.rollout_batched(E.MLP, net, x0, C, c, o["K"], o["k"], xs, u0, lo, hi, decay, max_ls)
    # the preconditions that let every problem and every point be compared, from the oracle's own outputs
    margin = np.nanmin(np.abs(trials - old2) / (1.0 + np.abs(old2)))
    assert margin >= 1e-6, "a line-search trial within %g of the nominal cost: the recipe changed" % margin
    if act != "sigmoid":
        kink = min(np.abs(h).min() for pts in ((xs, u0), (nx, nu))
                   for h in pre_activations(net, pts[0][:-1].reshape(-1, ns), pts[1][:-1].reshape(-1, nc)))
        assert kink >= 1e-8, "a hidden pre-activation within %g of the kink: the recipe changed" % kink
    if backtracks:
        assert (alphas < 1).any(), "no problem backtracks: the recipe changed"

    xk, ck = be.mlp_traj_cost(f64(x0), f64(u0), sp, C=f64(C), c=f64(c))
    close(host(xk), xs, "trajectory")
    np.testing.assert_allclose(host(ck), old, rtol=BAR)
    Fk, fk = be.mlp_linearize(sp, f64(xs[:-1].reshape(-1, ns)), f64(u0[:-1].reshape(-1, nc)))
    close(host(Fk), Fl, "F")
    close(host(fk), fl, "f")
    r = be.mlp_rollout(f64(x0), f64(C), f64(c), f64(o["K"]), f64(o["k"]), f64(xs), f64(u0), f64(old2),
                       StepOptions(u_lower=lo, u_upper=hi, linesearch_decay=decay, max_linesearch_iter=max_ls), sp)
    torch.cuda.synchronize()
    assert np.array_equal(host(r["alphas"]), running(alphas, decay))
    close(host(r["new_x"]), nx, "new_x")
    close(host(r["new_u"]), nu, "new_u")
    np.testing.assert_allclose(host(r["costs"]), costs, rtol=BAR)
    np.testing.assert_allclose(host(r["old_costs"]), old2, rtol=BAR)
    np.testing.assert_allclose(host(r["full_du_norm"]), full, rtol=BAR)
    taken = np.sqrt(((u0 - nu) ** 2).sum((0, 2)))
    np.testing.assert_allclose(host(r["alpha_du_norm"]), taken, rtol=BAR, atol=1e-300)
    assert (host(r["status"]) == 0).all()
    if bound is not None:
        assert (host(r["new_u"]) >= lo).all() and (host(r["new_u"]) <= hi).all()


# ---------------------------------------------------------------------------------------------
# 3. ctrl_carry
# ---------------------------------------------------------------------------------------------
def test_float64_rollout_carries_the_control(be):
    """MlpSpec.augmented() of a (4, 2, [16]) sigmoid network, rollout with gains, against the oracle on CtrlPassthroughDynamics
    semantics: state (u_prev, x), next (u, net(x, u))."""
    from mpc._native import StepOptions
    from oracle import env_oracle as E
    ns, nc, B, T = 4, 2, 7, 6
    inner = random_net(ns, nc, [16], "sigmoid", True, seed=402, scale=3.0)
    aug = spec_of(inner).augmented()
    assert aug.ctrl_carry == nc and aug.weights[0].dtype == torch.float64
    na, n = ns + nc, ns + 2 * nc
    rng = np.random.RandomState(B)
    z0 = rng.randn(B, na)
    u0 = 0.3 * rng.randn(T, B, nc)
    A = 0.3 * rng.randn(T, B, n, n)
    C = np.einsum("tbki,tbkj->tbij", A, A) + 0.1 * np.eye(n)
    c = rng.randn(T, B, n)
    K, k = 0.1 * rng.randn(T, B, nc, na), 0.3 * rng.randn(T, B, nc)
    orig = E.mlp_step

    def carry_step(z, u, net):
        return np.concatenate((np.asarray(u, dtype=np.float64), orig(np.asarray(z)[:, nc:], u, inner)), 1)
    E.mlp_step = carry_step
    try:
        zs = E.traj(E.MLP, z0, u0, inner)
        nx, nu, costs, full, alphas, trials, old = E.rollout_batched(E.MLP, inner, z0, C, c, K, k, zs, u0, -0.6, 0.6, 0.2, 5)
    finally:
        E.mlp_step = orig
    # (random gains, not a sweep's: the small-alpha trials sit close to the nominal by construction; a decision is safe while the
    # difference is far above the rounding of a float64 cost sum, 1e-15)
    assert np.nanmin(np.abs(trials - old) / (1.0 + np.abs(old))) >= 1e-10
    zk, _ = be.mlp_traj_cost(f64(z0), f64(u0), aug)
    close(host(zk), zs, "augmented trajectory")
    assert np.array_equal(host(zk)[1:, :, :nc], u0[:-1])                         # the control itself
    r = be.mlp_rollout(f64(z0), f64(C), f64(c), f64(K), f64(k), f64(zs), f64(u0), f64(old),
                       StepOptions(u_lower=-0.6, u_upper=0.6, linesearch_decay=0.2, max_linesearch_iter=5), aug)
    torch.cuda.synchronize()
    assert np.array_equal(host(r["alphas"]), running(alphas, 0.2))
    close(host(r["new_x"]), nx, "new_x")
    close(host(r["new_u"]), nu, "new_u")
    np.testing.assert_allclose(host(r["costs"]), costs, rtol=BAR)
    np.testing.assert_allclose(host(r["full_du_norm"]), full, rtol=BAR)


# ---------------------------------------------------------------------------------------------
# 4. edges
# ---------------------------------------------------------------------------------------------
def test_float64_edges(be):
    from mpc import _native
    from mpc._native import StepOptions
    from oracle import env_oracle as E
    L = _native.load()
    ns, nc = 5, 2
    n = ns + nc
    net = random_net(ns, nc, [9], "elu", True, seed=3, scale=2.0)
    sp = spec_of(net)
    rng = np.random.RandomState(0)
    # T = 1: no network call; B = 1
    x0, u0 = rng.randn(1, ns), rng.randn(1, 1, nc)
    C, c = np.eye(n)[None, None] * 2.0, rng.randn(1, 1, n)
    xk, ck = be.mlp_traj_cost(f64(x0), f64(u0), sp, C=f64(C), c=f64(c))
    assert np.array_equal(host(xk)[0], x0)
    np.testing.assert_allclose(host(ck), E.quad_cost(C, c, x0[None], u0), rtol=BAR)
    T = 5
    u0 = 0.3 * rng.randn(T, 1, nc)
    A = 0.3 * rng.randn(T, 1, n, n)
    C = np.einsum("tbki,tbkj->tbij", A, A) + 0.1 * np.eye(n)
    c = rng.randn(T, 1, n)
    xs = E.traj(E.MLP, x0, u0, net)
    K, k = 0.1 * rng.randn(T, 1, nc, ns), 0.3 * rng.randn(T, 1, nc)
    nx, nu, costs, full, alphas, trials, old = E.rollout_batched(E.MLP, net, x0, C, c, K, k, xs, u0, -0.5, 0.5, 0.2, 4)
    opts = StepOptions(u_lower=-0.5, u_upper=0.5, linesearch_decay=0.2, max_linesearch_iter=4)
    args = (f64(x0), f64(C), f64(c), f64(K), f64(k), f64(xs), f64(u0), f64(old), opts, sp)
    # outputs pre-filled with NaN are fully overwritten; two runs are bitwise equal
    ox, ou = torch.full((T, 1, ns), float("nan"), device=DEV, dtype=torch.float64), torch.full((T, 1, nc), float("nan"), device=DEV, dtype=torch.float64)
    r1 = be.mlp_rollout(*args, out_x=ox, out_u=ou)
    r2 = be.mlp_rollout(*args)
    torch.cuda.synchronize()
    close(host(ox), nx, "new_x")
    close(host(ou), nu, "new_u")
    for key in ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alpha_du_norm", "alphas"):
        assert torch.isfinite(r1[key]).all() and torch.equal(r1[key], r2[key]), key
    pts_x, pts_u = f64(xs[:-1].reshape(-1, ns)), f64(u0[:-1].reshape(-1, nc))
    N = pts_x.shape[0]
    oF = torch.full((N, ns, n), float("nan"), device=DEV, dtype=torch.float64)
    of = torch.full((N, ns), float("nan"), device=DEV, dtype=torch.float64)
    be.mlp_linearize(sp, pts_x, pts_u, out_F=oF, out_f=of)
    F2, f2 = be.mlp_linearize(sp, pts_x, pts_u)
    torch.cuda.synchronize()
    assert torch.isfinite(oF).all() and torch.equal(oF, F2) and torch.equal(of, f2)
    Fl, fl = E.linearize(E.MLP, xs[:-1].reshape(-1, ns), u0[:-1].reshape(-1, nc), net)
    close(host(oF), Fl, "F")
    close(host(of), fl, "f")
    # B = 0 and N = 0 return 0 and touch nothing
    e, ws, nbytes, keep = sp.to_struct(pts_x)
    p = _native.Problem()
    p.B, p.T, p.ns, p.nc, p.dtype = 0, T, ns, nc, _native.MPC_F64
    assert L.mpc_mlp_rollout_dtype(ctypes.byref(p), None, ctypes.byref(e), None, None, None, ctypes.byref(_native.Outputs()),
                                   ws.data_ptr(), nbytes, None) == 0
    assert L.mpc_mlp_linearize_dtype(ctypes.byref(e), _native.MPC_F64, ns, nc, 0, None, None, None, None, ws.data_ptr(), nbytes, None) == 0
    F0, f0 = be.mlp_linearize(sp, pts_x[:0], pts_u[:0])
    assert tuple(F0.shape) == (0, ns, n) and tuple(f0.shape) == (0, ns)


# ---------------------------------------------------------------------------------------------
# 5. whole solves
# ---------------------------------------------------------------------------------------------
def _solve_problem():
    from mpc.dynamics import NNDynamics
    ns, nc, B, T = 12, 4, 5, 8
    n = ns + nc
    torch.manual_seed(7)

    class ModulePath(NNDynamics):
        """The same network on the module path: `native_net` declines a subclass that overrides forward."""

        def forward(self, x, u):
            return super().forward(x, u)
    plain = NNDynamics(ns, nc, [100], activation="sigmoid").double().to(DEV)
    module = ModulePath(ns, nc, [100], activation="sigmoid").double().to(DEV)
    module.load_state_dict(plain.state_dict())
    rng = np.random.RandomState(11)
    A = 0.3 * rng.randn(T, B, n, n)
    C = f64(np.einsum("tbki,tbkj->tbij", A, A) + 0.1 * np.eye(n))
    c = f64(rng.randn(T, B, n))
    x_init = f64(rng.randn(B, ns))
    return (ns, nc, B, T), plain, module, x_init, C, c


def _controller(dims):
    from mpc import mpc
    ns, nc, B, T = dims
    return mpc.MPC(ns, nc, T, u_lower=-0.5, u_upper=0.5, lqr_iter=3, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                   grad_method=mpc.GradMethods.ANALYTIC)


def test_float64_solve_runs_in_the_kernels_and_matches_the_module_path(be, monkeypatch):
    from mpc import mpc
    from mpc.dynamics import NNDynamics
    dims, plain, module, x_init, C, c = _solve_problem()
    ctrl = _controller(dims)
    assert plain.native_net(x_init) is not None and module.native_net(x_init) is None
    assert ctrl.solve_route(x_init, mpc.QuadCost(C, c), plain).loop == "network"
    assert ctrl.solve_route(x_init, mpc.QuadCost(C, c), module).loop == "general"
    calls = {"forward": 0}
    orig = NNDynamics.forward

    def counted(self, x, u):
        calls["forward"] += 1
        return orig(self, x, u)
    monkeypatch.setattr(NNDynamics, "forward", counted)
    with torch.no_grad():
        x, u, costs = ctrl(x_init, mpc.QuadCost(C, c), plain)
    torch.cuda.synchronize()
    assert calls["forward"] == 0                                  # no Python call of the network during the solve
    with torch.no_grad():
        x2, u2, costs2 = _controller(dims)(x_init, mpc.QuadCost(C, c), module)
    torch.cuda.synchronize()
    assert calls["forward"] >= (dims[3] - 1) * 3                  # the module path calls it timestep by timestep
    close(host(x), host(x2), "x")
    close(host(u), host(u2), "u")
    np.testing.assert_allclose(host(costs), host(costs2), rtol=BAR)
    assert float(u.abs().max()) <= 0.5


def test_float64_solve_with_a_gradient_matches_the_module_path(be):
    from mpc import mpc
    dims, plain, module, x_init, C, c = _solve_problem()
    w = f64(np.random.RandomState(5).randn(dims[3], dims[2], dims[0] + dims[1]))
    got = []
    for dyn in (plain, module):
        xi = x_init.clone().requires_grad_(True)
        x, u, costs = _controller(dims)(xi, mpc.QuadCost(C, c), dyn)
        (torch.cat((x, u), 2) * w).sum().backward()
        got.append((host(x), host(u), host(costs), host(xi.grad)))
    torch.cuda.synchronize()
    for name, a, b in zip(("x", "u", "costs", "d loss / d x_init"), got[0], got[1]):
        if name == "costs":
            np.testing.assert_allclose(a, b, rtol=BAR)
        else:
            close(a, b, name)
    assert np.abs(got[0][3]).max() > 0
