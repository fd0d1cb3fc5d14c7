"""CPU-only: the float64 weight gradient of the NNDynamics linearisation (csrc/nn_param_grad64.h, mpc_mlp_param_grad_dtype,
HipBackend.mlp_linearize_backward64, mpc.MPC(f64_weight_grad_kernel=True)).

  (1) header against EXPORTS, the ABI number, the build-info tokens;
  (2) the entries' codes without a device in both dtypes, the query on the envelope, the workspace size;
  (3) the kernels' own statements run on the host by tests/nn64_grad_host.cpp -- 512 threads around a barrier are the block, the
      LDS stand-in is a heap block of exactly the planned size -- against the float64 yardstick (tests/nn_weight_grad_ref.py) and
      the reference-made fixture at |err_k| <= 1e-9 |g_k| + 1e-9 sum_points |contribution_k|;
  (4) the same file as a stand-alone program under the host sanitizers (address + undefined behaviour, thread);
  (5) the routing of MPC.linearize_dynamics / MPC.forward on a CPU stand-in backend that records `mlp_linearize_backward64`;
  (6) the kernels' code-object notes: no scratch, no spilled VGPRs.
"""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from mpc import _native, mpc
from mpc.dynamics import CtrlPassthroughDynamics
from mpc.mpc import GradMethods, QuadCost
from oracle_backend import OracleBackend

import nn_weight_grad_ref as R

CSRC = os.path.join(ROOT, "mpc.pytorch_amd", "csrc")
HOST_SRC = os.path.join(ROOT, "tests", "nn64_grad_host.cpp")
F32, F64 = 0, 1
BAR = 1e-9
ENTRIES = ("mpc_mlp_param_grad_supported_dtype", "mpc_mlp_param_grad_workspace_bytes_dtype", "mpc_mlp_param_grad_dtype")

# (n_state, n_ctrl, hidden, activation, passthrough, seed): the issue's list.  The relu (3, 1, [16, 16, 16]) network is drawn with
# seed 35 as in tests/test_gpu_nn_weight_grad.py
NETS = [(3, 1, [], "sigmoid", True, 34), (5, 2, [20], "sigmoid", True, 36), (5, 2, [20], "relu", True, 36),
        (6, 3, [40, 24], "sigmoid", True, 37), (6, 3, [40, 24], "relu", True, 37), (3, 1, [16, 16, 16], "sigmoid", True, 34),
        (3, 1, [16, 16, 16], "relu", False, 35), (17, 3, [33], "sigmoid", True, 48), (12, 4, [100], "sigmoid", True, 43),
        (12, 4, [100], "sigmoid", False, 43), (12, 4, [100], "relu", True, 43), (12, 4, [100], "relu", False, 43),
        (32, 8, [100], "sigmoid", True, 63)]
# past the staging limit: 20 236 weights and biases = 158 KiB, which no block holds beside its own area
IN_PLACE = (12, 4, [128, 128], "sigmoid", True, 71)
FIXTURE_CASES = (("s5", 5, 2, [20], "sigmoid", True), ("r5", 5, 2, [20], "relu", True), ("s6", 6, 3, [40, 24], "sigmoid", True),
                 ("r12", 12, 4, [100], "relu", False), ("lin3", 3, 1, [], "sigmoid", True))


def _net(widths, act=0, carry=0, ptr=16):
    e = _native.MlpDynamics()
    e.n_layers, e.activation, e.passthrough, e.ctrl_carry = len(widths) - 1, act, 1, carry
    for l, w in enumerate(widths[:5]):
        e.widths[l] = w
    for l in range(min(len(widths) - 1, 4)):
        e.W[l], e.b[l] = ptr, ptr
    return e


# ---------------------------------------------------------------------------------------------
# (1) header, exports, ABI
# ---------------------------------------------------------------------------------------------
def test_the_header_declares_the_entries_and_the_binding_loads_them():
    header = open(os.path.join(ROOT, "include", "mpc_lqr.h")).read()
    L = _native.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.EXPORTS and hasattr(L, name)
    assert "MPC_LQR_ABI_VERSION 9" in header and L.mpc_lqr_abi_version() == _native.ABI_VERSION == 9      # additive: the number stays
    info = L.mpc_lqr_build_info().decode()
    assert "nn_param_grad<f32>" in info and "nn_param_grad64" in info
    kernel_header = open(os.path.join(CSRC, "nn_param_grad64.h")).read()
    assert int(re.search(r"#define MPC_MLP_PARAM_GRAD64_MAX_BLOCKS (\d+)", kernel_header).group(1)) == _native.MLP_PARAM_GRAD64_MAX_BLOCKS
    assert int(re.search(r"PG64_THREADS = (\d+)", kernel_header).group(1)) == _native.MLP_PARAM_GRAD64_THREADS
    assert "nn_param_grad64.h" in open(os.path.join(CSRC, "nn_dynamics64.hip")).read()
    assert hasattr(_native.HipBackend, "mlp_linearize_backward64")


# ---------------------------------------------------------------------------------------------
# (2) codes, query and workspace size without a device
# ---------------------------------------------------------------------------------------------
def test_param_grad_dtype_refuses_before_a_launch():
    L = _native.load()
    e = _net([16, 100, 12])
    out = _native.MlpParamGrads()
    for l in range(2):
        out.gW[l], out.gb[l] = 16, 16
    hole = _native.MlpParamGrads()
    hole.gW[0], hole.gb[0], hole.gW[1] = 16, 16, 16
    for dtype in (F32, F64):          # the same codes in both dtypes
        need = L.mpc_mlp_param_grad_workspace_bytes_dtype(ctypes.byref(e), dtype, 1000)
        assert need > 0

        def call(net, ns, nc, N, x=16, u=16, gF=16, gf=16, o=out, ws=16, nbytes=need):
            return L.mpc_mlp_param_grad_dtype(ctypes.byref(net) if net is not None else None, dtype, ns, nc, N, x, u, gF, gf,
                                              ctypes.byref(o) if o is not None else None, ws, nbytes, None)
        assert call(e, 12, 4, -1) == -1 and call(e, 0, 4, 8) == -1 and call(e, 12, 0, 8) == -1         # MPC_E_DIMS
        assert call(None, 12, 4, 8) == -2 and call(e, 12, 4, 8, o=None) == -2 and call(e, 12, 4, 8, ws=None) == -2
        for k in ("x", "u", "gF", "gf"):
            assert call(e, 12, 4, 8, **{k: None}) == -2                                                 # MPC_E_NULL
        assert call(e, 12, 4, 8, o=hole) == -2                                                          # gb_2 NULL
        assert call(e, 11, 4, 8) == -1                                                                  # widths against n_state
        assert call(e, 12, 4, 1000, nbytes=need - 1) == -1 and b"workspace" in L.mpc_lqr_last_error()
        assert call(_net([16, 100, 12], carry=4), 12, 4, 8) == -1 and b"ctrl_carry" in L.mpc_lqr_last_error()
        assert call(_net([16, 100, 12], act=2), 12, 4, 8) == -1 and b"ELU" in L.mpc_lqr_last_error()
        assert call(_net([16, 2048, 12]), 12, 4, 8, nbytes=1 << 30) == -1 and b"outside" in L.mpc_lqr_last_error()
        assert call(_net([16, 100, 12], ptr=None), 12, 4, 8) == -1 and b"outside" in L.mpc_lqr_last_error()     # an incomplete description
        # N = 0 is a call like any other (it writes zeros): the same checks in front of it
        assert call(e, 12, 4, 0, o=None) == -2 and call(e, 12, 4, 0, nbytes=16) == -1
    assert L.mpc_mlp_param_grad_dtype(ctypes.byref(e), 7, 12, 4, 8, 16, 16, 16, 16, ctypes.byref(out), 16, 1 << 30, None) == -3      # MPC_E_DTYPE


def test_the_query_on_the_envelope():
    L = _native.load()
    S = lambda e, ns, nc, dtype=F64: int(L.mpc_mlp_param_grad_supported_dtype(ctypes.byref(e), ns, nc, dtype))
    for ns, nc, hidden in sorted(set((ns, nc, tuple(h)) for ns, nc, h, _, _, _ in NETS + [IN_PLACE])):
        for act in (0, 1):
            e = _net([ns + nc] + list(hidden) + [ns], act=act)
            assert S(e, ns, nc) == 1, (ns, nc, hidden)
            assert S(e, ns, nc, F32) == (1 if L.mpc_mlp_supported(ctypes.byref(e), ns, nc) & 4 else 0)
    assert S(_net([16, 100, 12]), 12, 4, F32) == 1 and S(_net([16, 1024, 12]), 12, 4, F32) == 0          # MPC_F32: bit 2
    assert S(_net([16, 100, 12], act=2), 12, 4) == 0                                 # ELU
    assert S(_net([16, 100, 12], carry=4), 12, 4) == 0                               # ctrl_carry
    assert S(_net([37, 100, 33]), 33, 4) == 0                                        # 33 states
    five = _net([16, 8, 8, 8, 12])
    five.n_layers = 5
    assert S(five, 12, 4) == 0                                                       # 5 layers
    assert S(_net([16, 100, 12], ptr=None), 12, 4) == 0                              # an incomplete description
    assert S(_net([16, 100, 12]), 12, 4, 7) == 0                                     # no such dtype
    assert S(_net([16, 100, 12]), 11, 4) == 0 and L.mpc_mlp_param_grad_supported_dtype(None, 12, 4, F64) == 0
    assert S(_net([16, 2048, 12]), 12, 4) == 0                                       # more weights than the widest instantiation owns
    # the rollout / linearisation query keeps its float64 answer (tests/test_nn_f64_host.py pins it)
    assert L.mpc_mlp_supported_dtype(ctypes.byref(_net([16, 100, 12])), 12, 4, F64) == 3
    dx = R.make_net(12, 4, [100], "sigmoid", True, seed=1, dtype=torch.float64)
    spec = _native.MlpSpec(*R.net_params(dx), "sigmoid", True)
    assert spec.param_grad_supported(torch.float64) and spec.param_grad_supported() and not spec.augmented().param_grad_supported(torch.float64)
    assert not _native.MlpSpec(spec.weights, spec.biases, "elu", True).param_grad_supported(torch.float64)


def kmax_of(L, e):
    """The KMAX instantiation the launcher picks: one block's partial is KMAX * 512 doubles (include/mpc_lqr.h)"""
    one = int(L.mpc_mlp_param_grad_workspace_bytes_dtype(ctypes.byref(e), F64, 1))
    assert one > 0 and one % (8 * _native.MLP_PARAM_GRAD64_THREADS) == 0
    return one // (8 * _native.MLP_PARAM_GRAD64_THREADS)


def test_workspace_bytes_dtype():
    L = _native.load()
    W = lambda e, dtype, N: int(L.mpc_mlp_param_grad_workspace_bytes_dtype(ctypes.byref(e) if e is not None else None, dtype, N))
    e = _net([16, 100, 12])
    cap = _native.MLP_PARAM_GRAD64_MAX_BLOCKS * _native.MLP_PARAM_GRAD64_BLOCK_POINTS
    sizes = [W(e, F64, n) for n in (0, 1, 2, 17, cap - 1, cap, cap + 1, 10 ** 9)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] == sizes[-2] == sizes[-3]      # the cap on the blocks
    assert sizes[-1] == cap * sizes[1] and sizes[2] == 2 * sizes[1]
    for n in (0, 1, 1000):
        assert W(e, F32, n) == L.mpc_mlp_param_grad_workspace_bytes(ctypes.byref(e), n)
    for bad in (_net([16, 100, 12], act=2), _net([16, 100, 12], carry=4), _net([16, 100, 12], ptr=None), _net([16, 2048, 12])):
        assert W(bad, F64, 8) == -1
    assert W(None, F64, 8) == -1 and W(e, 7, 8) == -1
    # the three instantiations, by the networks' weights and biases
    assert kmax_of(L, e) == 8 and kmax_of(L, _net([40, 100, 32])) == 16 and kmax_of(L, _net([16, 128, 128, 12])) == 40


# ---------------------------------------------------------------------------------------------
# (3) the kernels' statements on the host
# ---------------------------------------------------------------------------------------------
def _cxx():
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    return cxx if os.path.exists(cxx) else shutil.which("clang++")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _cxx()
    if not cxx:
        pytest.skip("needs clang++")
    so = os.path.join(tmp_path_factory.mktemp("nn64grad"), "libnn64_grad_host.so")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Wno-unused-function", "-I", CSRC, "-o", so, HOST_SRC])
    lib = ctypes.CDLL(so)
    vp, i, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.nn64_grad_host.argtypes = [lg, i, i, i, vp, vp, vp, vp, i, i, i, vp, vp, vp, i, vp, vp, vp]
    lib.nn64_grad_host_plan.argtypes = [i, vp, ctypes.POINTER(lg), ctypes.POINTER(lg)]
    return lib


ACT = {"sigmoid": 0, "relu": 1}


def host_grads(lib, Ws, bs, act, passthrough, x, u, gF, gf, staged, blocks):
    """The gradients as the kernels' statements compute them, `blocks` blocks; outputs and workspace full of NaN beforehand"""
    Wn = [np.ascontiguousarray(W.detach().numpy(), dtype=np.float64) for W in Ws]
    bn = [np.ascontiguousarray(b.detach().numpy(), dtype=np.float64) for b in bs]
    xn, un, gFn, gfn = (np.ascontiguousarray(t.numpy(), dtype=np.float64) for t in (x, u, gF, gf))
    widths = np.array([Wn[0].shape[1]] + [W.shape[0] for W in Wn], dtype=np.int32)
    Lh = len(Wn)
    kmax = lib.nn64_grad_host_plan(Lh, widths.ctypes.data, None, None)
    assert kmax in (8, 16, 40)
    partials = np.full(blocks * kmax * _native.MLP_PARAM_GRAD64_THREADS, np.nan)
    gW, gb = [np.full_like(W, np.nan) for W in Wn], [np.full_like(b, np.nan) for b in bn]
    arr = lambda ts: (ctypes.c_void_p * Lh)(*[t.ctypes.data for t in ts])
    N, ns = xn.shape
    rc = lib.nn64_grad_host(N, blocks, ns, un.shape[1], xn.ctypes.data, un.ctypes.data, gFn.ctypes.data, gfn.ctypes.data, Lh, ACT[act],
                            int(passthrough), widths.ctypes.data, arr(Wn), arr(bn), int(staged), partials.ctypes.data, arr(gW), arr(gb))
    assert rc == kmax
    return [torch.from_numpy(t) for pair in zip(gW, gb) for t in pair], kmax


WORST = {}


@pytest.fixture(scope="module")
def report():
    yield
    if WORST:
        print("\nworst err / limit on the host: %.3g (%s)" % max((v, k) for k, v in WORST.items()))


# ((32, 8, [100]) and the network past the staging limit run on the device, tests/test_gpu_nn_f64_grad.py: at 512 threads around a
# barrier their points take seconds each here; their instantiations, KMAX 16 and 40, run below on one point)
@pytest.mark.parametrize("ns,nc,hidden,act,passthrough,seed", [c for c in NETS if c[0] + c[1] <= 16 or c[2] == [33]])
def test_host_run_of_the_kernels_matches_the_yardstick(host, report, ns, nc, hidden, act, passthrough, seed):
    dx = R.make_net(ns, nc, hidden, act, passthrough, seed=seed, dtype=torch.float64)
    Ws, bs = R.net_params(dx)
    for N in (1, 3, 37):
        x, u, gF, gf, rejected = R.random_points(Ws, bs, act, N, seed=100 + N, dtype=torch.float64)
        assert rejected <= 0.25
        _, _, grads, scales = R.yardstick(Ws, bs, act, passthrough, x, u, gF, gf)
        for staged in (True, False):
            got, kmax = host_grads(host, Ws, bs, act, passthrough, x, u, gF, gf, staged, blocks=min(N, 3))
            assert kmax == 8
            worst = R.check(got, grads, scales, rel=BAR, ab=BAR)
            WORST[(ns, nc, tuple(hidden), act, N, staged)] = worst
            assert worst <= 1., (N, staged, worst)
        if N == 3:
            again, _ = host_grads(host, Ws, bs, act, passthrough, x, u, gF, gf, False, blocks=3)
            assert all(torch.equal(a, b) for a, b in zip(again, got)), "a second run returns other bits"


@pytest.mark.parametrize("ns,nc,hidden,act,passthrough,seed,kmax", [NETS[-1] + (16,), IN_PLACE + (40,)])
def test_host_run_of_the_wider_instantiations(host, report, ns, nc, hidden, act, passthrough, seed, kmax):
    dx = R.make_net(ns, nc, hidden, act, passthrough, seed=seed, dtype=torch.float64)
    Ws, bs = R.net_params(dx)
    x, u, gF, gf, _ = R.random_points(Ws, bs, act, 2, seed=5, dtype=torch.float64)
    _, _, grads, scales = R.yardstick(Ws, bs, act, passthrough, x, u, gF, gf)
    for staged in (True, False):
        got, k = host_grads(host, Ws, bs, act, passthrough, x, u, gF, gf, staged, blocks=2)
        assert k == kmax
        worst = R.check(got, grads, scales, rel=BAR, ab=BAR)
        WORST[(ns, nc, tuple(hidden), act, 2, staged)] = worst
        assert worst <= 1., (staged, worst)


@pytest.mark.parametrize("name,ns,nc,hidden,act,passthrough", FIXTURE_CASES)
def test_host_run_reproduces_the_reference_fixture(host, report, name, ns, nc, hidden, act, passthrough):
    """The reference's own float64 gradients (tests/golden/nn_weight_grad_f64.npz, loaded as tests/test_nn_weight_grad.py does)."""
    z = golden("nn_weight_grad_f64")
    L = len(hidden) + 1
    c = {k[len(name) + 1:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(name + "_")}
    Ws, bs = [c["W%d" % l] for l in range(L)], [c["b%d" % l] for l in range(L)]
    ref = [c[k % l] for l in range(L) for k in ("gW%d", "gb%d")]
    assert c["x"].shape[1] == ns and int(c["act"]) == ACT[act] and int(c["passthrough"]) == int(passthrough)
    _, _, _, scales = R.yardstick(Ws, bs, act, passthrough, c["x"], c["u"], c["gF"], c["gf"])
    N = c["x"].shape[0]
    for staged in (True, False):
        got, _ = host_grads(host, Ws, bs, act, passthrough, c["x"], c["u"], c["gF"], c["gf"], staged, blocks=min(N, 4))
        worst = R.check(got, ref, scales, rel=BAR, ab=BAR)
        WORST[("fixture " + name, staged)] = worst
        assert worst <= 1., (staged, worst)


def test_the_planned_lds_of_the_listed_networks_fits_a_workgroup(host):
    """area + staged network in bytes against 160 KiB, from the header's own layout functions; the network past the staging limit
    is one whose weights leave no room for its area"""
    def plan(ns, nc, hidden):
        widths = np.array([ns + nc] + list(hidden) + [ns], dtype=np.int32)
        area, staged = ctypes.c_long(), ctypes.c_long()
        kmax = host.nn64_grad_host_plan(len(widths) - 1, widths.ctypes.data, ctypes.byref(area), ctypes.byref(staged))
        return kmax, 8 * area.value, 8 * staged.value
    budget = 160 * 1024 - 256
    for ns, nc, hidden, _, _, _ in NETS:
        kmax, area, staged = plan(ns, nc, hidden)
        assert kmax and staged <= 96 * 1024 and area + staged <= budget, (ns, nc, hidden)
    kmax, area, staged = plan(*IN_PLACE[:3])
    assert kmax == 40 and area <= budget and staged > 96 * 1024 and area + staged > budget


# ---------------------------------------------------------------------------------------------
# (4) the same file, stand-alone, under the host sanitizers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_stand_alone_host_program_under_the_sanitizers(tmp_path, sanitizers):
    """tests/nn64_grad_host.cpp with its own main.  AddressSanitizer + UndefinedBehaviorSanitizer: the LDS stand-in is a heap
    block of exactly the doubles the launch plan gives a block, the partials exactly the workspace.  ThreadSanitizer: the block's
    threads are threads and `sync()` their only ordering, so a missing `sync()` is a reported race."""
    cxx = _cxx()
    if not cxx:
        pytest.skip("needs clang++")
    exe = str(tmp_path / "nn64_grad_host")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function",
                            "-fsanitize=" + sanitizers, "-fno-sanitize-recover=undefined", "-DNN64_GRAD_HOST_MAIN", "-I", CSRC, "-o", exe,
                            HOST_SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "nn64_grad_host: ok" in run.stdout, run.stdout + run.stderr


# ---------------------------------------------------------------------------------------------
# (5) routing on the oracle stand-in
# ---------------------------------------------------------------------------------------------
class Grad64Backend(OracleBackend):
    """The oracle stand-in plus `mlp_linearize` and a recording `mlp_linearize_backward64`, both answered by the yardstick; the
    float32 backward must never be asked."""

    def mlp_linearize(self, net, x, u, out_F=None, out_f=None):
        self.calls.append("mlp_linearize")
        F, f, _, _ = R.yardstick(net.weights, net.biases, net.activation, net.passthrough, x, u,
                                 torch.zeros(x.shape[0], x.shape[1], x.shape[1] + u.shape[1]), torch.zeros_like(x))
        return F.to(x.dtype), f.to(x.dtype)

    def mlp_linearize_backward(self, net, x, u, gF, gf):
        self.calls.append("mlp_linearize_backward")
        raise AssertionError("the float32 weight gradient was asked")

    def mlp_linearize_backward64(self, net, x, u, gF, gf):
        self.calls.append("mlp_linearize_backward64")
        assert all(t.dtype == torch.float64 for t in (x, u, gF, gf))
        _, _, grads, _ = R.yardstick(net.weights, net.biases, net.activation, net.passthrough, x, u, gF, gf)
        return grads


@pytest.fixture
def on_device(monkeypatch):
    """A CPU box stands in for the device: MlpSpec.supported keeps every test but `is_cuda`, in either dtype."""
    def supported(weights, activation, like, bits=3):
        return (like.dtype in (torch.float32, torch.float64) and 1 <= len(weights) <= 4 and activation in _native.ACT_CODES
                and all(W.dtype == like.dtype for W in weights)
                and _native.MlpSpec.widths_supported([weights[0].shape[1]] + [W.shape[0] for W in weights], bits, like.dtype))
    monkeypatch.setattr(_native.MlpSpec, "supported", staticmethod(supported))


def _hooked(dx):
    dx.register_forward_hook(lambda mod, args, out: None)
    return dx


def _overriding(dx):
    base = type(dx)
    dx.__class__ = type("Custom" + base.__name__, (base,), {"forward": lambda self, x, u: base.forward(self, x, u)})
    return dx


def _second_tensor(dx):
    dx.extra = torch.ones(1, requires_grad=True, dtype=torch.float64)
    return dx


def solve_and_grad(be, dtype=torch.float64, wrap=None, act="sigmoid", hidden=(12,), ns=4, nc=2, B=5, T=6, **flags):
    """d loss / d (weights, biases) of one solve through an NNDynamics of `dtype` on backend `be`"""
    prev = _native.set_backend_for_testing(be)
    try:
        g = torch.Generator().manual_seed(3)
        dx = R.make_net(ns, nc, hidden, act, True, seed=7, dtype=dtype)
        if wrap is not None:
            dx = wrap(dx)
        n = ns + nc
        A = torch.randn(T, B, n, n, generator=g, dtype=torch.float64).to(dtype)
        C = A.transpose(2, 3).matmul(A) + 0.1 * torch.eye(n, dtype=dtype)
        c = torch.randn(T, B, n, generator=g, dtype=torch.float64).to(dtype)
        x0 = torch.randn(B, ns, generator=g, dtype=torch.float64).to(dtype)
        u0 = 0.2 * torch.randn(T, B, nc, generator=g, dtype=torch.float64).to(dtype)
        ctrl = mpc.MPC(ns, nc, T, u_lower=-0.5, u_upper=0.5, lqr_iter=4, verbose=-1, exit_unconverged=False,
                       detach_unconverged=False, grad_method=GradMethods.ANALYTIC, u_init=u0, **flags)
        x, u, _ = ctrl(x0, QuadCost(C, c), dx)
        ((u ** 2).sum() + x[-1].pow(2).sum()).backward()
        grads = []
        for p in dx.fcs.parameters():
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape and torch.isfinite(p.grad).all()
            grads.append(p.grad.detach().clone().double())
        return grads
    finally:
        _native.set_backend_for_testing(prev)


def assert_same_grads(got, ref, tol=BAR):
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert float(b.abs().max()) > 0
        assert float((a - b).abs().max()) <= tol * (1. + float(b.abs().max()))


@pytest.mark.parametrize("act,hidden", [("sigmoid", (12,)), ("relu", (12,)), ("sigmoid", (10, 9)), ("sigmoid", ())])
def test_the_flag_routes_a_float64_network_through_the_backend(on_device, act, hidden):
    be = Grad64Backend()
    got = solve_and_grad(be, act=act, hidden=hidden, f64_weight_grad_kernel=True)
    assert be.calls.count("mlp_linearize_backward64") == 1 and "mlp_linearize_backward" not in be.calls
    off = Grad64Backend()
    ref = solve_and_grad(off, act=act, hidden=hidden)                                   # flag off: the module path, no call
    assert "mlp_linearize_backward64" not in off.calls and "mlp_linearize_backward" not in off.calls
    assert_same_grads(got, ref)
    only32 = Grad64Backend()
    assert_same_grads(solve_and_grad(only32, act=act, hidden=hidden, weight_grad_kernel=True), ref)     # the float32 flag alone: no call
    assert "mlp_linearize_backward64" not in only32.calls and "mlp_linearize_backward" not in only32.calls


def test_the_float64_flag_does_not_route_a_float32_network(on_device):
    be = Grad64Backend()
    got = solve_and_grad(be, dtype=torch.float32, f64_weight_grad_kernel=True)
    assert "mlp_linearize_backward64" not in be.calls and "mlp_linearize_backward" not in be.calls
    assert_same_grads(got, solve_and_grad(Grad64Backend(), dtype=torch.float32), tol=1e-4)


@pytest.mark.parametrize("wrap", (_hooked, _overriding, _second_tensor))
def test_modules_the_kernels_would_not_reproduce_stay_on_the_module_path(on_device, wrap):
    be = Grad64Backend()
    got = solve_and_grad(be, wrap=wrap, f64_weight_grad_kernel=True)
    assert "mlp_linearize_backward64" not in be.calls and "mlp_linearize" not in be.calls
    assert_same_grads(got, solve_and_grad(Grad64Backend(), wrap=wrap))


def test_linearize_dynamics_itself_takes_the_route(on_device):
    be = Grad64Backend()
    prev = _native.set_backend_for_testing(be)
    try:
        ns, nc, T, B = 5, 2, 5, 3
        dx = R.make_net(ns, nc, [20], "sigmoid", True, seed=9, dtype=torch.float64)
        Ws, bs = R.net_params(dx)
        N = (T - 1) * B
        x, u, gF, gf, _ = R.random_points(Ws, bs, "sigmoid", T * B, seed=2, dtype=torch.float64)
        xs, us = x.view(T, B, ns), u.view(T, B, nc)
        ctrl = mpc.MPC(ns, nc, T, grad_method=GradMethods.ANALYTIC, f64_weight_grad_kernel=True)
        F, f = ctrl.linearize_dynamics(xs, us, dx, diff=True)
        ((F * gF[:N].view_as(F)).sum() + (f * gf[:N].view_as(f)).sum()).backward()
        assert be.calls == ["mlp_linearize", "mlp_linearize_backward64"]
        _, _, grads, scales = R.yardstick(Ws, bs, "sigmoid", True, x[:N], u[:N], gF[:N], gf[:N])
        params = [p for pair in zip(Ws, bs) for p in pair]
        assert all(p.grad.dtype == torch.float64 for p in params)
        assert R.check([p.grad for p in params], grads, scales, rel=BAR, ab=BAR) <= 1.
        # a second backward through the function is refused
        F, f = ctrl.linearize_dynamics(xs, us, dx, diff=True)
        gW, = torch.autograd.grad(F.sum() + f.sum(), Ws[0], create_graph=True)
        with pytest.raises(RuntimeError):
            gW.sum().backward()
        # diff=False: the forward kernel, no backward call
        del be.calls[:]
        F2, _ = ctrl.linearize_dynamics(xs, us, dx, diff=False)
        assert not F2.requires_grad and be.calls == ["mlp_linearize"]
        # the paths that keep what they had
        del be.calls[:]
        mpc.MPC(ns, nc, T, grad_method=GradMethods.AUTO_DIFF, f64_weight_grad_kernel=True).linearize_dynamics(xs, us, dx, diff=True)
        assert mpc.MPC(ns, nc, 1, grad_method=GradMethods.ANALYTIC, f64_weight_grad_kernel=True)._param_grad_net(dx, xs[:1]) is None
        aug = CtrlPassthroughDynamics(dx)
        assert mpc.MPC(ns + nc, nc, T, grad_method=GradMethods.ANALYTIC, f64_weight_grad_kernel=True)._param_grad_net(
            aug, torch.zeros(T, B, ns + nc, dtype=torch.float64)) is None
        assert mpc.MPC(ns, nc, T, grad_method=GradMethods.ANALYTIC)._param_grad_net(dx, xs) is None
        assert mpc.MPC(ns, nc, T, grad_method=GradMethods.ANALYTIC, weight_grad_kernel=True)._param_grad_net(dx, xs) is None
        assert ctrl._param_grad_net(dx, xs) is not None
        elu = R.make_net(ns, nc, [20], "elu", True, seed=9, dtype=torch.float64)
        assert ctrl._param_grad_net(elu, xs) is None
        assert be.calls == []
        # a backend without the float64 method keeps the module path
        _native.set_backend_for_testing(OracleBackend())
        assert ctrl._param_grad_net(dx, xs) is None
    finally:
        _native.set_backend_for_testing(prev)


def test_the_keyword_is_off_by_default_and_sits_before_the_last_two():
    names = list(inspect.signature(mpc.MPC.__init__).parameters)
    assert names[-3:] == ["f64_weight_grad_kernel", "weight_grad_kernel", "planned_network_slew"]
    assert inspect.signature(mpc.MPC.__init__).parameters["f64_weight_grad_kernel"].default is False
    assert mpc.MPC(4, 2, 5).f64_weight_grad_kernel is False


def test_the_float32_backend_call_keeps_refusing_doubles_and_the_float64_one_floats():
    dyn = R.make_net(5, 2, [8], "sigmoid", True, seed=1, dtype=torch.float64)
    spec = _native.MlpSpec(*R.net_params(dyn), "sigmoid", True)
    be = _native.HipBackend()
    d = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(TypeError, match="float32 only"):
        be.mlp_linearize_backward(spec, d(6, 5), d(6, 2), d(6, 5, 7), d(6, 5))
    with pytest.raises(TypeError, match="float64 only"):
        be.mlp_linearize_backward64(spec, d(6, 5).float(), d(6, 2).float(), d(6, 5, 7).float(), d(6, 5).float())


# ---------------------------------------------------------------------------------------------
# (6) the kernels' code-object notes: registers only
# ---------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None, reason="needs hipcc")
def test_kernels_stay_in_registers():
    """.vgpr_spill_count and .private_segment_fixed_size of every nn64_param_grad kernel (weights staged or not, KMAX 8 / 16 / 40,
    and the final sum) are 0, and a block's 512 threads fit a compute unit."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    text = "\n".join(isa_lint.assembly("nn_dynamics64"))
    seen = []
    for block in text.split("- .agpr_count")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "nn64_param_grad" in nm:
            seen.append(nm)
            assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, nm
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, nm
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)) <= 256, nm          # two wavefronts a SIMD
    assert sum("nn64_param_grad_kernel" in n for n in seen) == 6 and sum("nn64_param_grad_final_kernel" in n for n in seen) == 1, seen
