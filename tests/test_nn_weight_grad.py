"""CPU tests of the NNDynamics linearisation's weight gradient (csrc/nn_param_grad.h, mpc_mlp_param_grad,
_native.MlpLinearizeFn): the float64 yardstick (tests/nn_weight_grad_ref.py) against the reference-made fixture and against
float64 autograd of the package's own module, the host wiring of MPC.forward on a CPU stand-in, the C entry's argument
checks, the new struct's layout and the kernels' code-object notes."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from mpc import _native, mpc
from mpc.dynamics import CtrlPassthroughDynamics, NNDynamics
from mpc.mpc import GradMethods, QuadCost
from oracle_backend import OracleBackend

import nn_weight_grad_ref as R

# name in the fixture, n_state, n_ctrl, hidden, activation, passthrough
FIXTURE_CASES = (("s5", 5, 2, [20], "sigmoid", True), ("r5", 5, 2, [20], "relu", True), ("s6", 6, 3, [40, 24], "sigmoid", True),
                 ("r12", 12, 4, [100], "relu", False), ("lin3", 3, 1, [], "sigmoid", True))


def fixture_case(z, name, L):
    c = {k[len(name) + 1:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(name + "_")}
    c["Ws"], c["bs"] = [c["W%d" % l] for l in range(L)], [c["b%d" % l] for l in range(L)]
    c["grads"] = [c[k % l] for l in range(L) for k in ("gW%d", "gb%d")]
    return c


@pytest.fixture(scope="module")
def fixture():
    return golden("nn_weight_grad_f64")


# ---------------------------------------------------------------------------------------------
# 1. the yardstick against the reference-made fixture and against the package's own module
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ns,nc,hidden,act,passthrough", FIXTURE_CASES)
def test_yardstick_reproduces_the_reference_fixture(fixture, name, ns, nc, hidden, act, passthrough):
    c = fixture_case(fixture, name, len(hidden) + 1)
    assert c["x"].shape[1] == ns and c["u"].shape[1] == nc and int(c["passthrough"]) == int(passthrough)
    assert [W.shape[0] for W in c["Ws"]] == hidden + [ns] and int(c["act"]) == (0 if act == "sigmoid" else 1)
    F, f, grads, scales = R.yardstick(c["Ws"], c["bs"], act, passthrough, c["x"], c["u"], c["gF"], c["gf"])
    np.testing.assert_allclose(F.numpy(), c["F"].numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(f.numpy(), c["f"].numpy(), rtol=1e-9, atol=1e-9)
    worst = R.check(c["grads"], grads, scales, rel=0., ab=1e-9)
    print(name, "yardstick against the fixture: worst err / (1e-9 scale) = %.3g" % worst)
    assert worst <= 1.
    for g, s in zip(grads, scales):
        assert (s >= g.abs() * (1 - 1e-12)).all()
    assert (scales[-1] > 0).all()


@pytest.mark.parametrize("ns,nc,hidden,act,passthrough", [
    (5, 2, [], "sigmoid", True), (5, 2, [20], "sigmoid", True), (5, 2, [20], "relu", False), (12, 4, [100], "sigmoid", False),
    (12, 4, [100], "relu", True), (6, 3, [40, 24], "sigmoid", True), (6, 3, [40, 24], "relu", True), (3, 1, [16, 16, 16], "sigmoid", True),
    (3, 1, [16, 16, 16], "relu", False), (17, 3, [33], "sigmoid", True)])
def test_yardstick_is_float64_autograd_of_the_packages_module(ns, nc, hidden, act, passthrough):
    dx = R.make_net(ns, nc, hidden, act, passthrough, seed=11, dtype=torch.float64)
    Ws, bs = R.net_params(dx)
    x, u, gF, gf, rejected = R.random_points(Ws, bs, act, 37, seed=5, dtype=torch.float64)
    assert rejected <= 0.25
    F, f, grads, scales = R.yardstick(Ws, bs, act, passthrough, x, u, gF, gf, chunk=16)
    Fa, fa, ga = R.module_autograd(dx, x, u, gF, gf)
    np.testing.assert_allclose(F.numpy(), Fa.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(f.numpy(), fa.numpy(), rtol=1e-9, atol=1e-9)
    assert R.check(ga, grads, scales, rel=0., ab=1e-9) <= 1.


def test_relu_rejection_keeps_at_least_three_quarters():
    """(12, 4, [100]): the widest hidden layer of the GPU tests, where most points are lost."""
    dx = R.make_net(12, 4, [100], "relu", True, seed=21)
    Ws, bs = R.net_params(dx)
    x, u, _, _, rejected = R.random_points(Ws, bs, "relu", 1025, seed=3)
    print("(12, 4, [100]) relu: %.1f %% of the drawn points rejected" % (100 * rejected))
    assert 0. < rejected <= 0.25 and x.shape[0] == 1025
    assert (R.hidden_preactivations(Ws, bs, "relu", x, u).abs() >= R.REL_H).all()


# ---------------------------------------------------------------------------------------------
# 2. host wiring: MPC.forward + backward on a CPU stand-in that has the backward
# ---------------------------------------------------------------------------------------------
class NetOracleBackend(OracleBackend):
    """The stock stand-in plus `mlp_linearize`, answered by the float64 yardstick."""

    def mlp_linearize(self, net, x, u, out_F=None, out_f=None):
        self.calls.append("mlp_linearize")
        F, f, _, _ = R.yardstick(net.weights, net.biases, net.activation, net.passthrough, x, u,
                                 torch.zeros(x.shape[0], x.shape[1], x.shape[1] + u.shape[1]), torch.zeros_like(x))
        return F.to(x.dtype), f.to(x.dtype)


class GradOracleBackend(NetOracleBackend):
    """... plus `mlp_linearize_backward`."""

    def mlp_linearize_backward(self, net, x, u, gF, gf):
        self.calls.append("mlp_linearize_backward")
        _, _, grads, _ = R.yardstick(net.weights, net.biases, net.activation, net.passthrough, x, u, gF, gf)
        return [g.to(torch.float32) for g in grads]


@pytest.fixture
def on_device(monkeypatch):
    """A CPU box stands in for the device: MlpSpec.supported keeps every test but `is_cuda` (as tests/test_host_logic.py does)."""
    def supported(weights, activation, like):
        return (like.dtype == torch.float32 and 1 <= len(weights) <= 4 and activation in _native.ACT_CODES
                and all(W.dtype == torch.float32 for W in weights)
                and _native.MlpSpec.widths_supported([weights[0].shape[1]] + [W.shape[0] for W in weights]))
    monkeypatch.setattr(_native.MlpSpec, "supported", staticmethod(supported))


def _hooked(dx):
    dx.register_forward_hook(lambda mod, args, out: None)
    return dx


def _overriding(dx):
    base = type(dx)
    dx.__class__ = type("Custom" + base.__name__, (base,), {"forward": lambda self, x, u: base.forward(self, x, u)})
    return dx


def _double(dx):
    return dx.double()


def _second_tensor(dx):
    dx.extra = torch.ones(1, requires_grad=True)
    return dx


def solve_and_grad(be, act="sigmoid", wrap=None, hidden=(12,), ns=4, nc=2, B=5, T=6, lqr_iter=4, dtype=torch.float32):
    """d loss / d (weights, biases) of one solve through an NNDynamics on backend `be`"""
    prev = _native.set_backend_for_testing(be)
    try:
        g = torch.Generator().manual_seed(3)
        dx = R.make_net(ns, nc, hidden, act, True, seed=7)
        if wrap is not None:
            dx = wrap(dx)
        dt = next(dx.parameters()).dtype
        n = ns + nc
        A = torch.randn(T, B, n, n, generator=g, dtype=torch.float64).to(dt)
        C = A.transpose(2, 3).matmul(A) + 0.1 * torch.eye(n, dtype=dt)
        c = torch.randn(T, B, n, generator=g, dtype=torch.float64).to(dt)
        x0 = torch.randn(B, ns, generator=g, dtype=torch.float64).to(dt)
        u0 = 0.2 * torch.randn(T, B, nc, generator=g, dtype=torch.float64).to(dt)
        ctrl = mpc.MPC(ns, nc, T, u_lower=-0.5, u_upper=0.5, lqr_iter=lqr_iter, verbose=-1, exit_unconverged=False,
                       detach_unconverged=False, grad_method=GradMethods.ANALYTIC, weight_grad_kernel=True, u_init=u0)
        x, u, _ = ctrl(x0, QuadCost(C, c), dx)
        ((u ** 2).sum() + x[-1].pow(2).sum()).backward()
        grads = []
        for p in dx.fcs.parameters():
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape and torch.isfinite(p.grad).all()
            grads.append(p.grad.detach().clone().double())
        return grads
    finally:
        _native.set_backend_for_testing(prev)


def assert_same_grads(got, ref):
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert float(b.abs().max()) > 0
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-3, atol=1e-4 * float(b.abs().max()))


@pytest.mark.parametrize("act,hidden", [("sigmoid", (12,)), ("relu", (12,)), ("sigmoid", (10, 9)), ("sigmoid", ())])
def test_mpc_routes_the_differentiable_linearisation_through_the_backend(on_device, act, hidden):
    """ANALYTIC with a trainable network: forward = mlp_linearize, backward = mlp_linearize_backward, exactly one call of it,
    and the module path's gradients (float32 solves: rtol 1e-3, atol 1e-4 max|g| per tensor)."""
    be = GradOracleBackend()
    got = solve_and_grad(be, act, hidden=hidden)
    assert be.calls.count("mlp_linearize_backward") == 1 and be.calls.count("mlp_linearize") == 1
    # the stock stand-in without the backward: the same iterations, the final linearisation through the module
    stock = NetOracleBackend()
    ref = solve_and_grad(stock, act, hidden=hidden)
    assert "mlp_linearize_backward" not in stock.calls and "mlp_linearize" not in stock.calls
    assert any(k.startswith("network_iteration") for k in stock.calls) and any(k.startswith("network_iteration") for k in be.calls)
    assert_same_grads(got, ref)


@pytest.mark.parametrize("wrap", (_hooked, _overriding, _double, _second_tensor))
def test_modules_the_kernels_would_not_reproduce_stay_on_the_module_path(on_device, wrap):
    be = GradOracleBackend()
    got = solve_and_grad(be, wrap=wrap)
    assert "mlp_linearize_backward" not in be.calls and "mlp_linearize" not in be.calls
    assert_same_grads(got, solve_and_grad(NetOracleBackend(), wrap=wrap))            # the backend without the backward: the same module path
    if wrap is not _double:
        assert_same_grads(got, solve_and_grad(GradOracleBackend()))                  # ... and what the route gives for the plain module


def test_elu_stays_on_the_module_path(on_device):
    """elu has no grad_input (mpc/dynamics.py:113-114): the module refuses, as before, and no kernel is asked."""
    be = GradOracleBackend()
    prev = _native.set_backend_for_testing(be)
    try:
        dx = R.make_net(4, 2, [12], "elu", True, seed=7)
        assert dx.native_net(torch.zeros(1)) is not None
        ctrl = mpc.MPC(4, 2, 5, grad_method=GradMethods.ANALYTIC, weight_grad_kernel=True)
        assert ctrl._param_grad_net(dx, torch.zeros(5, 3, 4)) is None
        with pytest.raises(AssertionError):
            ctrl.linearize_dynamics(torch.zeros(5, 3, 4), torch.zeros(5, 3, 2), dx, diff=True)
        assert be.calls == []
    finally:
        _native.set_backend_for_testing(prev)


def test_linearize_dynamics_itself_takes_the_route(on_device):
    """MPC.linearize_dynamics(diff=True) called directly: the function and the yardstick's gradients; diff=False, the other
    gradient methods, CtrlPassthroughDynamics, T = 1 and a network on the host keep the path they had."""
    be = GradOracleBackend()
    prev = _native.set_backend_for_testing(be)
    try:
        ns, nc, T, B = 5, 2, 5, 3
        dx = R.make_net(ns, nc, [20], "sigmoid", True, seed=9)
        Ws, bs = R.net_params(dx)
        N = (T - 1) * B
        x, u, gF, gf, _ = R.random_points(Ws, bs, "sigmoid", T * B, seed=2)
        xs, us = x.view(T, B, ns), u.view(T, B, nc)
        ctrl = mpc.MPC(ns, nc, T, grad_method=GradMethods.ANALYTIC, weight_grad_kernel=True)
        F, f = ctrl.linearize_dynamics(xs, us, dx, diff=True)
        ((F * gF[:N].view_as(F)).sum() + (f * gf[:N].view_as(f)).sum()).backward()
        assert be.calls == ["mlp_linearize", "mlp_linearize_backward"]
        _, _, grads, scales = R.yardstick(Ws, bs, "sigmoid", True, x[:N], u[:N], gF[:N], gf[:N])
        params = [p for pair in zip(Ws, bs) for p in pair]
        assert R.check([p.grad for p in params], grads, scales, rel=0., ab=1e-6) <= 1.        # (float32 rounding of the returned tensors)
        # a second backward through the function is refused
        F, f = ctrl.linearize_dynamics(xs, us, dx, diff=True)
        gW, = torch.autograd.grad(F.sum() + f.sum(), Ws[0], create_graph=True)
        with pytest.raises(RuntimeError):
            gW.sum().backward()
        # diff=False: the forward kernel as before, nothing asks for a gradient, no backward call
        del be.calls[:]
        F2, f2 = ctrl.linearize_dynamics(xs, us, dx, diff=False)
        assert not F2.requires_grad and be.calls == ["mlp_linearize"]
        assert torch.equal(F2, F.detach()) and torch.equal(f2, f.detach())
        # the other paths
        del be.calls[:]
        for method in (GradMethods.AUTO_DIFF, GradMethods.FINITE_DIFF):
            mpc.MPC(ns, nc, T, grad_method=method).linearize_dynamics(xs, us, dx, diff=True)
        assert mpc.MPC(ns, nc, 1, grad_method=GradMethods.ANALYTIC, weight_grad_kernel=True)._param_grad_net(dx, xs[:1]) is None
        aug = CtrlPassthroughDynamics(dx)
        assert mpc.MPC(ns + nc, nc, T, grad_method=GradMethods.ANALYTIC, weight_grad_kernel=True)._param_grad_net(aug, torch.zeros(T, B, ns + nc)) is None
        assert ctrl._param_grad_net(dx, xs.double()) is None
        assert be.calls == []
    finally:
        _native.set_backend_for_testing(prev)


def test_the_route_is_an_opt_in(on_device):
    """mpc.MPC without `weight_grad_kernel=True` (the default) keeps the module path for diff=True: measured slower than the
    module route at (32, 8, [100]) (docs/history/r10.md)."""
    be = GradOracleBackend()
    prev = _native.set_backend_for_testing(be)
    try:
        ns, nc, T, B = 5, 2, 4, 3
        dx = R.make_net(ns, nc, [20], "sigmoid", True, seed=9)
        x, u, _, _, _ = R.random_points(*R.net_params(dx), "sigmoid", T * B, seed=2)
        ctrl = mpc.MPC(ns, nc, T, grad_method=GradMethods.ANALYTIC)
        assert ctrl.weight_grad_kernel is False and ctrl._param_grad_net(dx, x.view(T, B, ns)) is None
        F, f = ctrl.linearize_dynamics(x.view(T, B, ns), u.view(T, B, nc), dx, diff=True)
        assert F.requires_grad and be.calls == []
        on = mpc.MPC(ns, nc, T, grad_method=GradMethods.ANALYTIC, weight_grad_kernel=True)
        F2, f2 = on.linearize_dynamics(x.view(T, B, ns), u.view(T, B, nc), dx, diff=True)
        assert be.calls == ["mlp_linearize"]
        np.testing.assert_allclose(F2.detach().numpy(), F.detach().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(f2.detach().numpy(), f.detach().numpy(), rtol=1e-5, atol=1e-6)
    finally:
        _native.set_backend_for_testing(prev)


def test_a_network_on_the_host_keeps_the_module_path():
    """Without the `on_device` stand-in MlpSpec.supported refuses host tensors: diff=True is the module, bit for bit the stock
    backend's result, and diff=False likewise."""
    ns, nc, T, B = 5, 2, 4, 3
    dx = R.make_net(ns, nc, [20], "sigmoid", True, seed=9)
    Ws, bs = R.net_params(dx)
    x, u, _, _, _ = R.random_points(Ws, bs, "sigmoid", T * B, seed=2)
    res = []
    for be in (GradOracleBackend(), OracleBackend()):
        prev = _native.set_backend_for_testing(be)
        try:
            ctrl = mpc.MPC(ns, nc, T, grad_method=GradMethods.ANALYTIC, weight_grad_kernel=True)
            Fd, fd = ctrl.linearize_dynamics(x.view(T, B, ns), u.view(T, B, nc), dx, diff=True)
            with torch.no_grad():          # (as MPC.forward's iterations call it)
                Fn, fn = ctrl.linearize_dynamics(x.view(T, B, ns), u.view(T, B, nc), dx, diff=False)
            assert Fd.requires_grad and not Fn.requires_grad and be.calls == []
            res.append((Fd.detach(), fd.detach(), Fn, fn))
        finally:
            _native.set_backend_for_testing(prev)
    assert all(torch.equal(a, b) for a, b in zip(*res))
    assert torch.equal(res[0][0], res[0][2]) and torch.equal(res[0][1], res[0][3])


# ---------------------------------------------------------------------------------------------
# 3. the C entry's argument checks and the struct (no device needed)
# ---------------------------------------------------------------------------------------------
def _net(widths, act=0, carry=0, ptr=16):
    e = _native.MlpDynamics()
    e.n_layers, e.activation, e.passthrough, e.ctrl_carry = len(widths) - 1, act, 1, carry
    for l, w in enumerate(widths):
        e.widths[l] = w
    for l in range(len(widths) - 1):
        e.W[l], e.b[l] = ptr, ptr
    return e


def test_entry_point_validates_arguments_without_gpu():
    L = _native.load()
    e = _net([16, 100, 12])
    out = _native.MlpParamGrads()
    for l in range(2):
        out.gW[l], out.gb[l] = 16, 16
    need = L.mpc_mlp_param_grad_workspace_bytes(ctypes.byref(e), 1000)
    assert need > L.mpc_mlp_workspace_bytes(ctypes.byref(e))

    def call(net, ns, nc, N, x=16, u=16, gF=16, gf=16, o=out, ws=16, nbytes=need):
        return L.mpc_mlp_param_grad(ctypes.byref(net) if net is not None else None, ns, nc, N, x, u, gF, gf,
                                    ctypes.byref(o) if o is not None else None, ws, nbytes, None)
    assert call(e, 12, 4, -1) == -1 and call(e, 0, 4, 8) == -1 and call(e, 12, 0, 8) == -1
    assert call(None, 12, 4, 8) == -2 and call(e, 12, 4, 8, o=None) == -2 and call(e, 12, 4, 8, ws=None) == -2
    for k in ("x", "u", "gF", "gf"):
        assert call(e, 12, 4, 8, **{k: None}) == -2
    hole = _native.MlpParamGrads()
    hole.gW[0], hole.gb[0], hole.gW[1] = 16, 16, 16
    assert call(e, 12, 4, 8, o=hole) == -2                                              # gb_2 NULL
    assert call(e, 11, 4, 8) == -1                                                      # widths against n_state
    assert call(e, 12, 4, 1000, nbytes=need - 1) == -1 and b"workspace" in L.mpc_lqr_last_error()
    assert call(_net([16, 100, 12], carry=4), 12, 4, 8) == -1 and b"ctrl_carry" in L.mpc_lqr_last_error()
    assert call(_net([16, 100, 12], act=2), 12, 4, 8) == -1 and b"ELU" in L.mpc_lqr_last_error()
    assert call(_net([16, 1024, 12]), 12, 4, 8, nbytes=1 << 30) == -1 and b"bit 2" in L.mpc_lqr_last_error()
    # N = 0 is a call like any other (it writes zeros): the same checks in front of it, x .. gf may be NULL
    assert call(e, 12, 4, 0, o=None) == -2 and call(e, 12, 4, 0, nbytes=16) == -1
    need0 = L.mpc_mlp_param_grad_workspace_bytes(ctypes.byref(e), 0)
    assert 0 < need0 <= need
    sizes = [L.mpc_mlp_param_grad_workspace_bytes(ctypes.byref(e), n) for n in (0, 1, 16, 17, 1000, 16384, 16385, 10 ** 9)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] == sizes[-2]     # the cap on the number of blocks
    assert L.mpc_mlp_param_grad_workspace_bytes(ctypes.byref(_net([16, 1024, 12])), 8) == -1
    assert L.mpc_mlp_param_grad_workspace_bytes(None, 8) == -1


def test_supported_gains_bit_2_and_keeps_bits_0_and_1():
    L = _native.load()
    S = lambda e, ns, nc: int(L.mpc_mlp_supported(ctypes.byref(e), ns, nc))
    # every network of the GPU tests
    for ns, nc, hidden in ((12, 4, [100]), (5, 2, [20]), (6, 3, [40, 24]), (3, 1, [16, 16, 16]), (3, 1, []), (17, 3, [33]), (32, 8, [100])):
        for act in (0, 1):
            assert S(_net([ns + nc] + hidden + [ns], act=act), ns, nc) == 7, (ns, nc, hidden)
    # a probe by widths alone (what callers older than the bit compare with == 3) answers in bits 0 and 1 as before
    assert S(_net([16, 100, 12], ptr=None), 12, 4) == 3
    assert S(_net([16, 100, 12], act=2), 12, 4) == 3 and S(_net([16, 100, 12], carry=4), 12, 4) == 3
    assert S(_net([40, 1024, 32]), 32, 8) == 1 and S(_net([49, 100, 33]), 33, 16) == 0
    assert S(_net([40, 256, 256, 32]), 32, 8) & 4 == 0                                   # more gW tiles than a wavefront keeps
    assert _native.MlpSpec.widths_supported([40, 100, 32]) and not _native.MlpSpec.widths_supported([40, 1024, 32])
    dx = NNDynamics(12, 4, [100])
    spec = _native.MlpSpec([l.weight for l in dx.fcs], [l.bias for l in dx.fcs], "sigmoid", True)
    assert spec.param_grad_supported() and not spec.augmented().param_grad_supported()
    assert not _native.MlpSpec(spec.weights, spec.biases, "elu", True).param_grad_supported()


def test_struct_layout_matches_the_header():
    text = open(os.path.join(ROOT, "include", "mpc_lqr.h")).read()
    body = re.search(r"typedef struct mpc_mlp_param_grads \{(.*?)\} mpc_mlp_param_grads;", text, re.S).group(1)
    fields = re.findall(r"void \*(\w+)\[MPC_MLP_MAX_LAYERS\];", body)
    assert fields == ["gW", "gb"] == [f[0] for f in _native.MlpParamGrads._fields_]
    assert int(re.search(r"#define MPC_MLP_MAX_LAYERS (\d+)", text).group(1)) == _native.MLP_MAX_LAYERS == 4
    assert ctypes.sizeof(_native.MlpParamGrads) == 2 * 4 * ctypes.sizeof(ctypes.c_void_p)
    assert _native.MlpParamGrads.gb.offset == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert "MPC_LQR_ABI_VERSION 9" in text and _native.ABI_VERSION == 9
    assert int(re.search(r"#define MPC_MLP_PARAM_GRAD_MAX_BLOCKS (\d+)", text).group(1)) == 256


# ---------------------------------------------------------------------------------------------
# 4. the kernels' code-object notes: registers only
# ---------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None, reason="needs hipcc")
def test_kernel_stays_in_registers():
    """.vgpr_spill_count and .private_segment_fixed_size of every nn_param_grad kernel (weights staged or not, 16 or 40 tiles,
    and the final sum) are 0."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    text = "\n".join(isa_lint.assembly("nn_dynamics"))
    seen = []
    for block in text.split("- .agpr_count")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "nn_param_grad" in nm:
            seen.append(nm)
            assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, nm
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, nm
    assert sum("nn_param_grad_kernel" in n for n in seen) == 4 and sum("nn_param_grad_final_kernel" in n for n in seen) == 1, seen
