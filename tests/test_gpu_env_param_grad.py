"""GPU tests (-m gpu) of mpc_env_param_grad / _native.EnvLinearizeFn: the gradient of the simulator linearisation (F, f) with
respect to the simulator's parameters, one kernel over the (T-1) B trajectory points (csrc/env_param_grad.hip).

Yardstick: float64 torch autograd through the package's own `_transition` with create_graph=True
(tests/env_param_grad_ref.py; tests/test_env_param_grad.py ties it to the reference-made fixture at 1e-9), evaluated at
the inputs the kernel gets (the float32-rounded ones for the float32 kernel).  Tolerances, with scale_k = sum over the
points of |the point's contribution to g_k|:
    float64   |err_k| <= 1e-9 scale_k
    float32   |err_k| <= 1e-3 |g_k| + 1e-4 scale_k"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from mpc import _native

import env_param_grad_ref as R
import test_env_param_grad as cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float64, torch.float32)
CAP_POINTS = 512 * 256          # blocks under the cap x points per block: one more point and the stride loop wraps


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()            # fail loudly if the extension is missing
    return _native.HipBackend()


def spec(kind, dtype):
    prm = torch.tensor(R.PARAMS[kind], dtype=dtype, device=DEV)
    return R.make_dx(kind, prm).native_env(), prm


def raw_call(env, x, u, gF, gf):
    """mpc_env_param_grad itself, output and workspace pre-filled with NaN"""
    L = _native.load()
    N = x.shape[0]
    nbytes = int(L.mpc_env_param_grad_workspace_bytes(N))
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((env.n_params,), float("nan"), dtype=x.dtype, device=DEV)
    e, keep = env.to_struct(x)
    rc = L.mpc_env_param_grad(ctypes.byref(e), _native._dtype_code(x), N, x.data_ptr(), u.data_ptr(), gF.data_ptr(), gf.data_ptr(),
                              out.data_ptr(), ws.data_ptr(), nbytes, _native._stream(x.device))
    assert rc == 0, L.mpc_lqr_last_error()
    torch.cuda.synchronize()
    return out


def check(got, g64, scale, dtype, what):
    err = (got.double() - g64).abs()
    bound = 1e-9 * scale if dtype == torch.float64 else 1e-3 * g64.abs() + 1e-4 * scale
    print(what, "err / scale", (err / scale).tolist())
    assert torch.isfinite(got).all() and (err <= bound).all(), (what, got, g64, scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("kind", R.KINDS)
def test_kernel_on_the_reference_fixture(be, kind, dtype):
    c = cpu.fixture_case(golden("env_param_grad_f64"), kind)
    prm, x, u, gF, gf = (c[k].to(dtype).to(DEV) for k in ("params", "x", "u", "gF", "gf"))
    env = R.make_dx(kind, prm).native_env()
    got = be.env_linearize_backward(env, x, u, gF, gf)
    assert got.dtype == dtype and got.is_cuda and got.shape == (len(R.PARAMS[kind]),)
    if dtype == torch.float64:
        g64, scale = c["gparams"].to(DEV), R.yardstick(kind, prm, x, u, gF, gf)[3]
    else:
        _, _, g64, scale = R.yardstick(kind, prm, x, u, gF, gf)
    check(got, g64, scale, dtype, "%s fixture" % kind)


@functools.lru_cache(maxsize=None)
def _points(kind, N, dtype):
    x, u, gF, gf = R.random_points(kind, N, 100 + N % 97, DEV, dtype)
    _, _, g64, scale = R.yardstick(kind, torch.tensor(R.PARAMS[kind], dtype=dtype), x, u, gF, gf)
    return x, u, gF, gf, g64, scale


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("kind", R.KINDS)
def test_kernel_on_random_points(be, kind, dtype):
    """A partial wavefront, a partial block, several blocks, and one point more than the capped grid covers in one pass;
    a fifth of the controls outside the clamp and two exactly on it; NaN in the output and the workspace beforehand; the
    same bits from a second call."""
    env, _ = spec(kind, dtype)
    u_max = env.u_max
    for N in (1, 63, 64, 65, 257, CAP_POINTS + 1):
        x, u, gF, gf, g64, scale = _points(kind, N, dtype)
        if N >= 63:
            outside = float((u.abs() > u_max).double().mean())
            assert 0.1 < outside < 0.3 and (u == u_max).any() and (u == -u_max).any()
        got = raw_call(env, x, u, gF, gf)
        check(got, g64, scale, dtype, "%s N=%d" % (kind, N))
        again = raw_call(env, x, u, gF, gf)
        assert torch.equal(got, again), (N, got, again)
        assert torch.equal(be.env_linearize_backward(env, x, u, gF, gf), got)
    assert torch.equal(be.env_linearize_backward(env, x[:0], u[:0], gF[:0], gf[:0]), torch.zeros_like(got))     # N = 0


@functools.lru_cache(maxsize=None)
def _module_route(kind):
    return cpu.solve_and_grad(kind, None, wrap=cpu._hidden, B=16, T=12, device=DEV)


@pytest.mark.parametrize("where", ("cpu", DEV))
@pytest.mark.parametrize("kind", R.KINDS)
def test_whole_solve_gradient_matches_the_module_route(be, monkeypatch, kind, where):
    """float64 MPC.forward + backward with params.requires_grad, AUTO_DIFF: the kernel route (iterations and the final
    differentiable linearisation on the device) against the module route (native_env hidden); the backward kernel runs
    exactly once; the gradient arrives where `params` lives (solve_and_grad asserts device and dtype)."""
    real = _native.backend()
    assert isinstance(real, _native.HipBackend)
    ran = []
    orig = real.env_linearize_backward
    monkeypatch.setattr(real, "env_linearize_backward", lambda *a: (ran.append(1), orig(*a))[1], raising=False)
    got = cpu.solve_and_grad(kind, None, B=16, T=12, device=DEV, params_device=where)
    assert len(ran) == 1
    ref = _module_route(kind)
    assert len(ran) == 1
    assert got.device.type == torch.device(where).type
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=1e-6)


def test_the_backward_is_once_differentiable(be):
    """Asking for a double backward through the function raises (it must not return zeros)."""
    kind = "pendulum_full"
    x, u, gF, gf = R.random_points(kind, 65, 9, DEV, torch.float64)
    prm = torch.tensor(R.PARAMS[kind], dtype=torch.float64, device=DEV, requires_grad=True)
    env = R.make_dx(kind, prm).native_env()
    F, f = _native.EnvLinearizeFn.apply(prm, env, x, u)
    assert F.requires_grad and f.requires_grad
    g, = torch.autograd.grad((F * gF).sum() + (f * gf).sum(), prm, retain_graph=True)
    _, _, g64, scale = R.yardstick(kind, prm, x, u, gF, gf)
    check(g, g64, scale, torch.float64, "EnvLinearizeFn")
    # a loss whose cotangents depend on the parameters themselves: its second derivative would need the backward's own
    g2, = torch.autograd.grad((F * gF).sum() * (f * gf).sum(), prm, create_graph=True)
    assert g2.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g2.sum().backward()
