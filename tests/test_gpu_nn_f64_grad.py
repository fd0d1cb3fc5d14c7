"""GPU tests of mpc_mlp_param_grad_dtype(MPC_F64) / HipBackend.mlp_linearize_backward64 / mpc.MPC(f64_weight_grad_kernel=True):
the kernels of csrc/nn_param_grad64.h against the float64 yardstick (tests/nn_weight_grad_ref.py, held to the reference-made
fixture by tests/test_nn_weight_grad.py) at the project's float64 bar, |err_k| <= 1e-9 |g_k| + 1e-9 sum_points |contribution_k|,
the reference's own recorded gradients, and whole float64 solves against the module route.

Measured worst err / limit on one MI355X: docs/history/r32.md."""
import ctypes

import pytest
import torch

from conftest import golden
from mpc import _native, mpc
from mpc.mpc import GradMethods, QuadCost

import nn_weight_grad_ref as R
from test_nn_f64_grad_host import BAR, FIXTURE_CASES, IN_PLACE, NETS, kmax_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
CAP = _native.MLP_PARAM_GRAD64_MAX_BLOCKS * _native.MLP_PARAM_GRAD64_BLOCK_POINTS        # points of one pass of the grid
# the KMAX instantiation each network takes (asserted from the workspace query)
KMAX = {(32, 8, (100,)): 16, (12, 4, (128, 128)): 40}


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available()
    return _native.HipBackend()


def spec_of(Ws, bs, act, passthrough):
    return _native.MlpSpec([W.detach().to(DEV) for W in Ws], [b.detach().to(DEV) for b in bs], act, passthrough)


def run_kernel(spec, x, u, gF, gf):
    """mpc_mlp_param_grad_dtype(MPC_F64) through the C ABI with outputs and workspace full of NaN beforehand; (gradients on the
    host, KMAX of the launch)."""
    L = _native.load()
    x, u, gF, gf = (t.to(DEV).contiguous() for t in (x, u, gF, gf))
    N, ns = x.shape
    nc = u.shape[1]
    e, _, _, keep = spec.to_struct(x)
    assert L.mpc_mlp_param_grad_supported_dtype(ctypes.byref(e), ns, nc, _native.MPC_F64) == 1
    nbytes = int(L.mpc_mlp_param_grad_workspace_bytes_dtype(ctypes.byref(e), _native.MPC_F64, N))
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.full((nbytes // 8,), float("nan"), device=DEV, dtype=F64)
    out, grads = _native.MlpParamGrads(), []
    for l, (W, b) in enumerate(zip(spec.weights, spec.biases)):
        gW, gb = torch.full_like(W, float("nan")), torch.full_like(b, float("nan"))
        out.gW[l], out.gb[l] = gW.data_ptr(), gb.data_ptr()
        grads += [gW, gb]
    rc = L.mpc_mlp_param_grad_dtype(ctypes.byref(e), _native.MPC_F64, ns, nc, N, x.data_ptr(), u.data_ptr(), gF.data_ptr(), gf.data_ptr(),
                                    ctypes.byref(out), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.mpc_lqr_last_error()
    torch.cuda.synchronize()
    return [g.cpu() for g in grads], kmax_of(L, e)


def against_yardstick(be, Ws, bs, act, passthrough, x, u, gF, gf, what, kmax):
    spec = spec_of(Ws, bs, act, passthrough)
    assert spec.param_grad_supported(F64)
    _, _, grads, scales = R.yardstick(Ws, bs, act, passthrough, x, u, gF, gf)
    got, k = run_kernel(spec, x, u, gF, gf)
    assert k == kmax, (what, k)
    assert all(torch.isfinite(g).all() and g.dtype == F64 for g in got)
    worst = R.check(got, grads, scales, rel=BAR, ab=BAR)
    print("%s: worst err / limit = %.3g" % (what, worst))
    assert worst <= 1., what
    # the backend method is the C call, bit for bit -- and so a second call returns the same bits
    again = be.mlp_linearize_backward64(spec, x.to(DEV), u.to(DEV), gF.to(DEV), gf.to(DEV))
    torch.cuda.synchronize()
    assert all(a.dtype == F64 and torch.equal(a.cpu(), b) for a, b in zip(again, got)), "mlp_linearize_backward64 returns other bits"
    return worst


@pytest.mark.parametrize("ns,nc,hidden,act,passthrough,seed", NETS + [IN_PLACE])
def test_kernel_against_the_float64_yardstick(be, ns, nc, hidden, act, passthrough, seed):
    dx = R.make_net(ns, nc, hidden, act, passthrough, seed=seed, dtype=F64)
    Ws, bs = R.net_params(dx)
    if (ns, nc, hidden) == (32, 8, [100]):
        sizes = (1, 17, 1025)
    elif (ns, nc, hidden) == (5, 2, [20]):
        sizes = (1, 3, CAP, CAP + 1, 1025)
    else:
        sizes = (1, 3, 1025)
    for N in sizes:
        x, u, gF, gf, rejected = R.random_points(Ws, bs, act, N, seed=100 + N, dtype=F64)
        assert rejected <= 0.25
        against_yardstick(be, Ws, bs, act, passthrough, x, u, gF, gf, "(%d, %d, %s) %s N = %d" % (ns, nc, hidden, act, N),
                          KMAX.get((ns, nc, tuple(hidden)), 8))


@pytest.mark.parametrize("name,ns,nc,hidden,act,passthrough", FIXTURE_CASES)
def test_the_reference_fixture_through_the_kernel(be, name, ns, nc, hidden, act, passthrough):
    """The reference's own case against the reference's own recorded float64 gradients (scale from the yardstick)."""
    z = golden("nn_weight_grad_f64")
    L = len(hidden) + 1
    c = {k[len(name) + 1:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(name + "_")}
    Ws, bs = [c["W%d" % l] for l in range(L)], [c["b%d" % l] for l in range(L)]
    ref = [c[k % l] for l in range(L) for k in ("gW%d", "gb%d")]
    _, _, grads, scales = R.yardstick(Ws, bs, act, passthrough, c["x"], c["u"], c["gF"], c["gf"])
    got, _ = run_kernel(spec_of(Ws, bs, act, passthrough), c["x"], c["u"], c["gF"], c["gf"])
    worst = R.check(got, ref, scales, rel=BAR, ab=BAR)
    print("fixture %s: worst err / limit = %.3g" % (name, worst))
    assert worst <= 1. and R.check(got, grads, scales, rel=BAR, ab=BAR) <= 1.


def test_no_points_gives_zeros(be):
    dx = R.make_net(5, 2, [20], "sigmoid", True, seed=1, dtype=F64)
    Ws, bs = R.net_params(dx)
    e = lambda *s: torch.empty(*s, dtype=F64)
    got, _ = run_kernel(spec_of(Ws, bs, "sigmoid", True), e(0, 5), e(0, 2), e(0, 5, 7), e(0, 5))
    assert all(bool((g == 0).all()) and g.shape == p.shape for g, p in zip(got, [t for pair in zip(Ws, bs) for t in pair]))


@pytest.mark.parametrize("ns,nc,hidden,bound", [(12, 4, [100], None), (12, 4, [100], 0.5), (6, 3, [40, 24], None)])
def test_whole_float64_solves_have_the_module_routes_gradients(be, monkeypatch, ns, nc, hidden, bound):
    """Flag on against flag off in the same process: the forward is identical, only the ending differs."""
    B, T, n = 16, 8, ns + nc
    g = torch.Generator().manual_seed(4)
    A = torch.randn(T, B, n, n, generator=g, dtype=F64)
    C = (A.transpose(2, 3).matmul(A) + 0.1 * torch.eye(n, dtype=F64)).to(DEV)
    c = torch.randn(T, B, n, generator=g, dtype=F64).to(DEV)
    x0 = torch.randn(B, ns, generator=g, dtype=F64).to(DEV)
    u0 = (0.2 * torch.randn(T, B, nc, generator=g, dtype=F64)).to(DEV)
    calls = []
    orig = _native.HipBackend.mlp_linearize_backward64

    def spy(self, *a):
        calls.append("mlp_linearize_backward64")
        return orig(self, *a)
    monkeypatch.setattr(_native.HipBackend, "mlp_linearize_backward64", spy)

    def solve(flag, double_backward=False):
        prev = _native.set_backend_for_testing(be)
        try:
            dx = R.make_net(ns, nc, hidden, "sigmoid", True, seed=13, dtype=F64).to(DEV)
            kw = {} if bound is None else dict(u_lower=-bound, u_upper=bound)
            ctrl = mpc.MPC(ns, nc, T, lqr_iter=3, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                           grad_method=GradMethods.ANALYTIC, f64_weight_grad_kernel=flag, u_init=u0.clone(), **kw)
            x, u, _ = ctrl(x0, QuadCost(C, c), dx)
            loss = (u ** 2).sum() + (u * torch.linspace(-1, 1, nc, device=DEV, dtype=F64)).sum()
            params = list(dx.fcs.parameters())
            if double_backward:
                gr = torch.autograd.grad(loss, params, create_graph=True)
                with pytest.raises(RuntimeError):
                    sum(t.sum() for t in gr).backward()
                return None, None
            loss.backward()
            torch.cuda.synchronize()
            assert all(p.grad is not None and p.grad.device == p.device and p.grad.dtype == F64 for p in params)
            return [p.grad.detach().cpu() for p in params], u.detach().cpu()
        finally:
            _native.set_backend_for_testing(prev)

    got, u_on = solve(True)
    assert calls == ["mlp_linearize_backward64"]
    ref, u_off = solve(False)
    assert calls == ["mlp_linearize_backward64"] and torch.equal(u_on, u_off)
    for a, b in zip(got, ref):
        assert torch.isfinite(a).all() and float(b.abs().max()) > 0
        err = float((a - b).abs().max())
        print("(%d, %d, %s) bound %s: max |diff| / (1 + max |g|) = %.3g" % (ns, nc, hidden, bound, err / (1. + float(b.abs().max()))))
        assert err <= BAR * (1. + float(b.abs().max()))
    solve(True, double_backward=True)
