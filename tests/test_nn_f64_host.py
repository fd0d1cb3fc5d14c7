"""CPU-only: float64 NNDynamics in the kernels (csrc/nn_dynamics64.hip, the mpc_mlp_*_dtype entries).

  (a) the new entries' codes without a device, mpc_mlp_supported_dtype on the envelope, header against EXPORTS;
  (b) what must KEEP today's route in float64: the weight gradient, the planned network slew loop, and the two float32-only
      backend calls, which refuse a double tensor loudly instead of casting it;
  (c) the kernels' own statements (csrc/nn_dynamics64.h) run on the host by tests/nn64_host.cpp -- sixty-four threads around a
      barrier stand in for the wavefront -- against oracle/env_oracle.py at the float64 bar, 1e-9 (1 + max |reference|);
  (d) the same file as a stand-alone program under the host sanitizers (address + undefined behaviour, thread).
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from mpc import _native, mpc
from mpc.dynamics import CtrlPassthroughDynamics, NNDynamics
from mpc.mpc import GradMethods, QuadCost
from oracle import env_oracle as E
from oracle import lqr_oracle as O
from oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc.pytorch_amd", "csrc")
HOST_SRC = os.path.join(ROOT, "tests", "nn64_host.cpp")
F32, F64 = 0, 1
BAR = 1e-9

# (n_state, n_ctrl, hidden): the networks the float64 kernels must take
ENVELOPE = [(12, 4, [100]), (32, 8, [100]), (5, 1, [64, 48]), (16, 8, [40, 32, 20]), (3, 2, []), (17, 3, [24, 24])]


def _net(ns, nc, hidden=(100,), pointers=16):
    e = _native.MlpDynamics()
    widths = [ns + nc] + list(hidden) + [ns]
    e.n_layers, e.activation, e.passthrough = len(widths) - 1, 0, 1
    for l, w in enumerate(widths):
        e.widths[l] = w
    for l in range(len(widths) - 1):
        e.W[l], e.b[l] = pointers, pointers
    return e


# ---------------------------------------------------------------------------------------------
# (a) the C entries without a device
# ---------------------------------------------------------------------------------------------
def test_the_header_declares_the_entries_and_the_binding_loads_them():
    header = open(os.path.join(ROOT, "include", "mpc_lqr.h")).read()
    L = _native.load()
    for name in ("mpc_mlp_supported_dtype", "mpc_mlp_workspace_bytes_dtype", "mpc_mlp_rollout_dtype", "mpc_mlp_linearize_dtype"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.EXPORTS and hasattr(L, name)
    assert L.mpc_lqr_abi_version() == _native.ABI_VERSION == 9                     # additive: the number stays
    info = L.mpc_lqr_build_info().decode()
    assert "nn_rollout<f32,f64>" in info and "nn_linearize<f32,f64>" in info and "nn_param_grad<f32>" in info


def test_supported_dtype_on_the_envelope():
    L = _native.load()
    for ns, nc, hidden in ENVELOPE:
        e = _net(ns, nc, hidden, pointers=None)
        assert L.mpc_mlp_supported_dtype(ctypes.byref(e), ns, nc, F64) == 3, (ns, nc, hidden)
        # ... bits 0 and 1 only, also for a complete description (bit 2, the weight gradient, is float32's)
        assert L.mpc_mlp_supported_dtype(ctypes.byref(_net(ns, nc, hidden)), ns, nc, F64) == 3
        # MPC_F32 is the existing entry
        for probe in (e, _net(ns, nc, hidden)):
            assert L.mpc_mlp_supported_dtype(ctypes.byref(probe), ns, nc, F32) == L.mpc_mlp_supported(ctypes.byref(probe), ns, nc)
    assert L.mpc_mlp_supported(ctypes.byref(_net(12, 4)), 12, 4) == 7                         # (the float32 answer has bit 2)
    for ns, nc, hidden in ((33, 4, [100]), (12, 4, [5000])):                                  # outside: the module path
        assert L.mpc_mlp_supported_dtype(ctypes.byref(_net(ns, nc, hidden, pointers=None)), ns, nc, F64) == 0
    five = _net(12, 4, [8, 8, 8], pointers=None)
    five.n_layers = 5
    assert L.mpc_mlp_supported_dtype(ctypes.byref(five), 12, 4, F64) == 0
    # the linearisation's chain buffers must fit a workgroup's LDS: 2 * 32 * 1024 doubles do not, the rollout's areas do
    assert L.mpc_mlp_supported_dtype(ctypes.byref(_net(32, 8, [1024, 1024, 64], pointers=None)), 32, 8, F64) == 1
    assert L.mpc_mlp_supported_dtype(ctypes.byref(_net(12, 4)), 11, 4, F64) == 0              # widths against n_state
    assert L.mpc_mlp_supported_dtype(ctypes.byref(_net(12, 4)), 12, 4, 7) == 0                # no such dtype
    assert L.mpc_mlp_supported_dtype(None, 12, 4, F64) == 0
    W = _native.MlpSpec.widths_supported
    assert W([16, 100, 12], dtype=torch.float64) and W([40, 1024, 1024, 64, 32], bits=1, dtype=torch.float64)
    assert not W([40, 1024, 1024, 64, 32], dtype=torch.float64) and not W([49, 100, 33], bits=1, dtype=torch.float64)
    assert W([16, 100, 12]) and not W([40, 1024, 32])                                         # float32: as before


def test_workspace_bytes_dtype():
    L = _native.load()
    e = _net(12, 4)
    assert L.mpc_mlp_workspace_bytes_dtype(ctypes.byref(e), F32) == L.mpc_mlp_workspace_bytes(ctypes.byref(e)) > 0
    assert L.mpc_mlp_workspace_bytes_dtype(ctypes.byref(e), F64) > 0
    assert L.mpc_mlp_workspace_bytes_dtype(ctypes.byref(_native.MlpDynamics()), F64) == 0    # no layers
    assert L.mpc_mlp_workspace_bytes_dtype(ctypes.byref(e), 7) == 0


def test_linearize_dtype_refuses_before_a_launch():
    L = _native.load()
    e = _net(12, 4)
    big = 1 << 20
    call = lambda e, dtype, ns, nc, N, x=16, ws=16, nbytes=big: L.mpc_mlp_linearize_dtype(
        ctypes.byref(e) if e is not None else None, dtype, ns, nc, N, x, 16, 16, 16, ws, nbytes, None)
    for dtype in (F32, F64):          # the same codes in both dtypes
        assert call(e, dtype, 12, 4, 0) == 0                                         # N = 0: nothing to do
        assert call(e, dtype, 12, 4, 0, x=None, ws=None, nbytes=0) == 0
        assert call(e, dtype, 12, 4, -1) == -1
        assert call(e, dtype, 0, 4, 8) == -1
        assert call(e, dtype, 12, 4, 8, x=None) == -2                                # MPC_E_NULL
        assert call(None, dtype, 12, 4, 8) == -2
        assert call(e, dtype, 12, 4, 8, ws=None, nbytes=0) == -5                     # no workspace
        assert b"workspace" in L.mpc_lqr_last_error()
        assert call(e, dtype, 12, 4, 8, ws=24) == -5                                 # misaligned
        assert call(e, dtype, 12, 4, 8, nbytes=8) == -5                              # short
        assert call(e, dtype, 11, 4, 8) == -1                                        # widths against n_state
        assert call(_net(33, 4), dtype, 33, 4, 8) == -1
        unset = _net(12, 4, pointers=None)
        assert call(unset, dtype, 12, 4, 8) == -2                                    # weight pointers NULL
        carry = _net(12, 4)
        carry.ctrl_carry = 4
        assert call(carry, dtype, 12, 4, 8) == -5 and b"ctrl_carry" in L.mpc_lqr_last_error()
        bad = _net(12, 4)
        bad.activation = 3
        assert call(bad, dtype, 12, 4, 8) == -5
    assert call(e, 7, 12, 4, 8) == -3                                                # MPC_E_DTYPE
    assert call(_net(32, 8, [1024, 1024, 64]), F64, 32, 8, 8) == -1 and b"too wide" in L.mpc_lqr_last_error()


def test_rollout_dtype_refuses_before_a_launch():
    L = _native.load()
    e = _net(12, 4)
    big = 1 << 20

    def problem(dtype, B=4, T=5, ns=12, nc=4, filled=True):
        p = _native.Problem()
        p.B, p.T, p.ns, p.nc, p.dtype = B, T, ns, nc, dtype
        if filled:
            p.x_init = p.C = p.c = p.cur_x = p.cur_u = 16
        return p

    def outputs(filled=True):
        out = _native.Outputs()
        if filled:
            out.new_x = out.new_u = out.costs = 16
        return out

    def call(p, out, net=e, o=None, K=None, k=None, old=None, ws=16, nbytes=big):
        return L.mpc_mlp_rollout_dtype(ctypes.byref(p), ctypes.byref(o) if o is not None else None, ctypes.byref(net), K, k, old,
                                       ctypes.byref(out) if out is not None else None, ws, nbytes, None)
    for dtype in (F32, F64):
        assert call(problem(dtype, B=0, filled=False), outputs(False)) == 0          # B = 0 succeeds and writes nothing
        assert call(problem(dtype, T=0), outputs()) == -1
        assert call(problem(dtype, filled=False), outputs()) == -2                   # x_init NULL
        assert call(problem(dtype), outputs(False)) == -2                            # new_x NULL
        assert call(problem(dtype), None) == -2
        assert call(problem(dtype), outputs(), K=16) == -2                           # K without k
        assert call(problem(dtype), outputs(), K=16, k=16) == -2                     # gains without old_costs
        o = _native.Options()
        o.max_linesearch_iter, o.delta_u = 0, float("nan")
        assert call(problem(dtype), outputs(), o=o, K=16, k=16, old=16) == -5        # max_linesearch_iter
        o.max_linesearch_iter = 10
        env = _native.EnvDynamics()
        env.kind, env.params, env.dt, env.u_max = _native.ENV_PENDULUM, 16, 0.05, 2.0
        o.true_dynamics = ctypes.pointer(env)
        assert call(problem(dtype, ns=3, nc=1), outputs(), net=_net(3, 1), o=o, K=16, k=16, old=16) == -5
        assert b"true_dynamics" in L.mpc_lqr_last_error()
        assert call(problem(dtype), outputs(), ws=None, nbytes=0) == -5              # workspace
        assert call(problem(dtype), outputs(), ws=24) == -5
        assert call(problem(dtype), outputs(), nbytes=8) == -5
        assert call(problem(dtype, ns=11), outputs()) == -1                          # widths against n_state
        carry = _net(12, 4)
        carry.ctrl_carry = 3
        assert call(problem(dtype), outputs(), net=carry) == -5                      # ctrl_carry must be n_ctrl
        assert call(problem(dtype), outputs(), net=_net(12, 4, pointers=None)) == -2
    assert call(problem(7), outputs()) == -3                                         # neither dtype


# ---------------------------------------------------------------------------------------------
# (b) float64 keeps today's route where only float32 kernels exist
# ---------------------------------------------------------------------------------------------
class _Kernels64(OracleBackend):
    """The oracle stand-in that says what HipBackend says about its augmented linearisation (float32 only) and records
    which network calls reach it."""
    carry_linearize_dtypes = _native.HipBackend.carry_linearize_dtypes

    def mlp_linearize_backward(self, net, x, u, gF, gf):
        self.calls.append("mlp_linearize_backward")
        raise AssertionError("the float32 weight gradient was asked for a float64 network")


@pytest.fixture
def any_widths(monkeypatch):
    """MlpSpec.supported refuses a CPU tensor before it looks at the widths: answer for it (tests/test_nn_slew_planned.py)."""
    monkeypatch.setattr(_native.MlpSpec, "supported", staticmethod(lambda weights, activation, like, bits=3: True))


def test_hip_backend_names_float32_for_the_augmented_linearisation():
    assert _native.HipBackend.carry_linearize_dtypes == (torch.float32,)


def test_float64_weight_gradient_keeps_the_module_path(any_widths):
    be = _Kernels64()
    prev = _native.set_backend_for_testing(be)
    try:
        ns, nc, T, B = 5, 2, 4, 3
        dx = NNDynamics(ns, nc, [8]).double()
        ctrl = mpc.MPC(ns, nc, T, grad_method=GradMethods.ANALYTIC, weight_grad_kernel=True)
        x = torch.zeros(T, B, ns, dtype=torch.float64)
        assert ctrl._param_grad_net(dx, x) is None
        assert ctrl._param_grad_net(dx.float(), x.float()) is not None               # (float32: the route it had)
        dx = dx.double()
        F, f = ctrl.linearize_dynamics(x, torch.zeros(T, B, nc, dtype=torch.float64), dx, diff=True)
        F.sum().backward()                                                           # torch autograd, not the kernel
        assert dx.fcs[0].weight.grad is not None and dx.fcs[0].weight.grad.dtype == torch.float64
        assert "mlp_linearize_backward" not in be.calls
    finally:
        _native.set_backend_for_testing(prev)


def test_float64_planned_network_slew_keeps_the_general_loop(any_widths):
    T, B, ns, nc = 4, 3, 5, 2
    n = ns + nc

    def plan(be, dtype):
        ctrl = mpc.MPC(ns, nc, T, slew_rate_penalty=0.5, planned_network_slew=True, grad_method=GradMethods.ANALYTIC)
        cost = QuadCost(torch.eye(n, dtype=dtype).expand(T, B, n, n), torch.zeros(T, B, n, dtype=dtype))
        dyn = NNDynamics(ns, nc, [8]).to(dtype)
        x0 = torch.zeros(B, ns, dtype=dtype)
        return ctrl._slew_plan(cost, dyn, be, x0), ctrl.solve_route(x0, cost, dyn) if be is _native.backend() else None
    be = _Kernels64()
    prev = _native.set_backend_for_testing(be)
    try:
        spec, route = plan(be, torch.float32)
        assert isinstance(spec, _native.MlpSpec) and spec.ctrl_carry == nc and route.loop == "slew"
        spec, route = plan(be, torch.float64)
        assert spec is None and route.loop == "general"
    finally:
        _native.set_backend_for_testing(prev)
    # a backend that names no dtypes takes every one (the stand-ins of tests/test_nn_slew_planned.py)
    be = OracleBackend()
    prev = _native.set_backend_for_testing(be)
    try:
        assert isinstance(plan(be, torch.float64)[0], _native.MlpSpec)
    finally:
        _native.set_backend_for_testing(prev)


def test_the_float32_only_backend_calls_refuse_a_double_tensor():
    """mlp_linearize_carry / mlp_linearize_backward used to cast to float32: a float64 caller gets an error, before anything
    touches the device (checked here through the dtype test alone: these tensors live on the host)."""
    dyn = NNDynamics(5, 2, [8]).double()
    spec = _native.MlpSpec([l.weight for l in dyn.fcs], [l.bias for l in dyn.fcs], "sigmoid", True)
    be = _native.HipBackend()
    z, u = torch.zeros(6, 7, dtype=torch.float64), torch.zeros(6, 2, dtype=torch.float64)
    x = torch.zeros(6, 5, dtype=torch.float64)
    for call in (lambda: be.mlp_linearize_carry(spec, z, u),
                 lambda: be.mlp_linearize_backward(spec, x, u, torch.zeros(6, 5, 7, dtype=torch.float64), torch.zeros(6, 5, dtype=torch.float64))):
        with pytest.raises((TypeError, RuntimeError), match="float32 only"):
            call()


def test_native_net_asks_for_one_dtype(monkeypatch):
    """MlpSpec.supported: network and `like` in the same dtype, on the device (a host tensor keeps the module path)."""
    asked = []
    monkeypatch.setattr(_native.MlpSpec, "widths_supported", staticmethod(lambda widths, bits=3, dtype=torch.float32: asked.append(dtype) or True))

    class OnDevice:
        """What MlpSpec.supported looks at in a tensor."""

        def __init__(self, dtype, shape=(1, 1)):
            self.is_cuda, self.dtype, self.shape = True, dtype, shape
    S = _native.MlpSpec.supported
    w = lambda dt: [OnDevice(dt, (8, 7)), OnDevice(dt, (5, 8))]
    assert S(w(torch.float64), "sigmoid", OnDevice(torch.float64)) and asked == [torch.float64]
    assert S(w(torch.float32), "sigmoid", OnDevice(torch.float32)) and asked == [torch.float64, torch.float32]
    assert not S(w(torch.float32), "sigmoid", OnDevice(torch.float64)) and not S(w(torch.float64), "sigmoid", OnDevice(torch.float32))
    assert not S(w(torch.float16), "sigmoid", OnDevice(torch.float16))
    dyn = NNDynamics(5, 2, [8]).double()
    assert dyn.native_net(torch.zeros(3, 5, dtype=torch.float64)) is None            # on the host
    assert CtrlPassthroughDynamics(dyn).native_net(torch.zeros(3, 7, dtype=torch.float64)) is None
    assert len(asked) == 2


# ---------------------------------------------------------------------------------------------
# (c) the kernels' statements on the host against the oracle
# ---------------------------------------------------------------------------------------------
def _cxx():
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    return cxx if os.path.exists(cxx) else shutil.which("clang++")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _cxx()
    if not cxx:
        pytest.skip("needs clang++")
    so = os.path.join(tmp_path_factory.mktemp("nn64"), "libnn64_host.so")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Wno-unused-function", "-I", CSRC, "-o", so, HOST_SRC])
    lib = ctypes.CDLL(so)
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.nn64_host_rollout.argtypes = [i] * 4 + [vp] * 8 + [i, d, d, vp, vp, vp, d, d, i] + [i] * 4 + [vp] * 3 + [i] + [vp] * 7
    lib.nn64_host_linearize.argtypes = [ctypes.c_long, i, i, vp, vp, i, i, i, vp, vp, vp, i, vp, vp]
    return lib


ACT = {"sigmoid": 0, "relu": 1, "elu": 2}


def _ptr(a):
    return None if a is None else a.ctypes.data


def _net_args(net, carry=0):
    Ws = [np.ascontiguousarray(W) for W in net.Ws]
    bs = [np.ascontiguousarray(b) for b in net.bs]
    widths = np.array([Ws[0].shape[1]] + [W.shape[0] for W in Ws], dtype=np.int32)
    Wp = (ctypes.c_void_p * len(Ws))(*[W.ctypes.data for W in Ws])
    bp = (ctypes.c_void_p * len(bs))(*[b.ctypes.data for b in bs])
    return (len(Ws), ACT[net.activation], int(net.passthrough), carry, widths, Wp, bp), (Ws, bs, widths, Wp, bp)


def host_rollout(lib, net, x0, C, c, cur_x, cur_u, K, k, old, lo, hi, decay, max_ls, staged, delta_u=None, u_zero_I=None, carry=0):
    T, B, nc = cur_u.shape
    ns = x0.shape[1]
    (L, act, pas, cr, widths, Wp, bp), keep = _net_args(net, carry)
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    x0, C, c, cur_x, cur_u, K, k, old = (arr(a) for a in (x0, C, c, cur_x, cur_u, K, k, old))
    mode, lo_s, hi_s, lo_a, hi_a = 0, 0.0, 0.0, None, None
    if lo is not None:
        if isinstance(lo, np.ndarray):
            mode, lo_a, hi_a = 2, arr(lo), arr(hi)
        else:
            mode, lo_s, hi_s = 1, float(lo), float(hi)
    zm = None if u_zero_I is None else np.ascontiguousarray(u_zero_I, dtype=np.uint8)
    # outputs pre-filled with NaN: everything the kernel reports must be overwritten
    out = dict(new_x=np.full((T, B, ns), np.nan), new_u=np.full((T, B, nc), np.nan), costs=np.full(B, np.nan),
               full_du_norm=np.full(B, np.nan), alpha_du_norm=np.full(B, np.nan), alphas=np.full(B, np.nan),
               status=np.zeros(B, dtype=np.int32))
    gains = K is not None
    rc = lib.nn64_host_rollout(B, T, ns, nc, _ptr(x0), _ptr(C), _ptr(c), _ptr(cur_x), _ptr(cur_u), _ptr(K), _ptr(k), _ptr(old), mode, lo_s,
                               hi_s, _ptr(lo_a), _ptr(hi_a), _ptr(zm), -1.0 if delta_u is None else float(delta_u), decay, max_ls,
                               L, act, pas, cr, widths.ctypes.data, Wp, bp, int(staged), _ptr(out["new_x"]),
                               _ptr(out["new_u"]) if gains else None, _ptr(out["costs"]) if C is not None else None,
                               _ptr(out["full_du_norm"]) if gains else None, _ptr(out["alpha_du_norm"]) if gains else None,
                               _ptr(out["alphas"]) if gains else None, _ptr(out["status"]))
    assert rc == 0
    return out


def host_linearize(lib, net, x, u, staged):
    N, ns = x.shape
    nc = u.shape[1]
    (L, act, pas, _, widths, Wp, bp), keep = _net_args(net)
    x, u = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
    F, f = np.full((N, ns, ns + nc), np.nan), np.full((N, ns), np.nan)
    assert lib.nn64_host_linearize(N, ns, nc, _ptr(x), _ptr(u), L, act, pas, widths.ctypes.data, Wp, bp, int(staged), _ptr(F), _ptr(f)) == 0
    return F, f


def random_net(ns, nc, hidden, act, passthrough, seed, scale=1.0):
    """tests/test_gpu_nn.py's recipe."""
    rng = np.random.RandomState(seed)
    sizes = [ns + nc] + list(hidden) + [ns]
    Ws = [scale * rng.uniform(-1, 1, (o, i)) / np.sqrt(i) for i, o in zip(sizes, sizes[1:])]
    bs = [rng.uniform(-1, 1, o) / np.sqrt(i) for i, o in zip(sizes, sizes[1:])]
    return E.Mlp(Ws, bs, act, passthrough)


def running(alphas, decay):
    """The oracle's alpha of trial i is decay ** i; the kernels, like the reference (mpc/lqr_step.py:247), keep the running
    product alpha *= decay, which is another double from i = 4 on (0.2: one ulp).  The oracle's trial, in the kernels' arithmetic."""
    table = np.cumprod(np.concatenate(([1.0], np.full(16, decay))))
    return table[np.rint(np.log(alphas) / np.log(decay)).astype(int)]


def close(got, want, what):
    err = np.abs(got - want).max()
    assert err <= BAR * (1.0 + np.abs(want).max()), (what, err)


# small batches (the host wavefront is sixty-four threads around a barrier), every code path: a bare layer, a layer wider than a
# wavefront, two and three hidden layers, one control, every activation, with and without passthrough, a box, none
HOST_CASES = [
    (3, 2, [], "sigmoid", True, 3, 5, None, 3.0, 0.3),
    (12, 4, [100], "sigmoid", True, 4, 6, 0.5, 5.0, 0.2),
    (5, 1, [64, 48], "relu", True, 5, 6, 2.0, 3.0, 0.3),
    (16, 8, [40, 32, 20], "elu", False, 3, 4, 1.0, 3.0, 0.3),
    (17, 3, [24, 24], "relu", True, 3, 5, 0.7, 3.0, 0.3),
    (12, 4, [128, 128], "relu", True, 3, 4, 0.5, 3.0, 0.3),           # past what a block stages on the device
]


@pytest.mark.parametrize("staged", [True, False])
@pytest.mark.parametrize("ns,nc,hidden,act,passthrough,B,T,bound,s,a", HOST_CASES)
def test_host_run_of_the_kernels_matches_the_oracle(host, ns, nc, hidden, act, passthrough, B, T, bound, s, a, staged):
    net = random_net(ns, nc, hidden, act, passthrough, seed=100 * ns + nc, scale=s)
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
    r = host_rollout(host, net, x0, C, c, None, u0, None, None, None, None, None, 0.2, 1, staged)
    close(r["new_x"], xs, "trajectory")
    np.testing.assert_allclose(r["costs"], old, rtol=BAR)
    Fl, fl = E.linearize(E.MLP, xs[:-1].reshape(-1, ns), u0[:-1].reshape(-1, nc), net)
    Fk, fk = host_linearize(host, net, xs[:-1].reshape(-1, ns), u0[:-1].reshape(-1, nc), staged)
    close(Fk, Fl, "F")
    close(fk, fl, "f")
    lo, hi = (None, None) if bound is None else (-bound, bound)
    o = O.lqr_step(x0, C, c, Fl.reshape(T - 1, B, ns, n), fl.reshape(T - 1, B, ns), xs, u0, lo, hi, linesearch_decay=0.2,
                   max_linesearch_iter=6, lockstep=False, return_gains=True)
    nx, nu, costs, full, alphas, trials, old2 = E.rollout_batched(E.MLP, net, x0, C, c, o["K"], o["k"], xs, u0, lo, hi, 0.2, 6)
    margin = np.nanmin(np.abs(trials - old2) / (1.0 + np.abs(old2)))
    assert margin >= 1e-6, margin                                       # no trial is a coin toss in float64
    r = host_rollout(host, net, x0, C, c, xs, u0, o["K"], o["k"], old2, lo, hi, 0.2, 6, staged)
    assert np.array_equal(r["alphas"], running(alphas, 0.2))
    close(r["new_x"], nx, "new_x")
    close(r["new_u"], nu, "new_u")
    np.testing.assert_allclose(r["costs"], costs, rtol=BAR)
    np.testing.assert_allclose(r["full_du_norm"], full, rtol=BAR)
    assert not np.isnan(r["alpha_du_norm"]).any() and (r["status"] == 0).all()


def test_host_run_honours_zero_mask_tensor_bounds_and_delta_u(host):
    ns, nc, B, T = 6, 3, 4, 6
    n = ns + nc
    net = random_net(ns, nc, [20], "sigmoid", True, seed=5, scale=3.0)
    rng = np.random.RandomState(1)
    x0 = rng.randn(B, ns)
    u0 = np.clip(0.3 * rng.randn(T, B, nc), -0.5, 0.5)
    A = 0.3 * rng.randn(T, B, n, n)
    C = np.einsum("tbki,tbkj->tbij", A, A) + 0.1 * np.eye(n)
    c = rng.randn(T, B, n)
    xs = E.traj(E.MLP, x0, u0, net)
    lo = -0.5 - 0.2 * rng.rand(T, B, nc)
    hi = 0.5 + 0.2 * rng.rand(T, B, nc)
    zero = rng.rand(T, B, nc) < 0.2
    K, k = 0.2 * rng.randn(T, B, nc, ns), 0.4 * rng.randn(T, B, nc)
    nx, nu, costs, full, alphas, trials, old = E.rollout_batched(E.MLP, net, x0, C, c, K, k, xs, u0, lo, hi, 0.2, 5, delta_u=0.15,
                                                                 u_zero_I=zero)
    assert np.nanmin(np.abs(trials - old) / (1.0 + np.abs(old))) >= 1e-6 and (alphas < 1).any()
    r = host_rollout(host, net, x0, C, c, xs, u0, K, k, old, lo, hi, 0.2, 5, True, delta_u=0.15, u_zero_I=zero)
    assert np.array_equal(r["alphas"], running(alphas, 0.2))
    close(r["new_u"], nu, "new_u")
    close(r["new_x"], nx, "new_x")
    np.testing.assert_allclose(r["costs"], costs, rtol=BAR)
    np.testing.assert_allclose(r["full_du_norm"], full, rtol=BAR)


def test_host_run_carries_the_control(host):
    """ctrl_carry: MlpSpec.augmented() of a (4, 2, [16]) network against CtrlPassthroughDynamics semantics in the oracle --
    state (u_prev, x), next (u, net(x, u))."""
    ns, nc, B, T = 4, 2, 3, 5
    inner = random_net(ns, nc, [16], "sigmoid", True, seed=402, scale=3.0)
    spec = _native.MlpSpec([torch.from_numpy(W) for W in inner.Ws], [torch.from_numpy(b) for b in inner.bs], "sigmoid", True).augmented()
    aug = E.Mlp([W.numpy() for W in spec.weights], [b.numpy() for b in spec.biases], "sigmoid", True)
    na, n = ns + nc, ns + 2 * nc
    rng = np.random.RandomState(B)
    z0 = rng.randn(B, na)
    u0 = 0.3 * rng.randn(T, B, nc)
    A = 0.3 * rng.randn(T, B, n, n)
    C = np.einsum("tbki,tbkj->tbij", A, A) + 0.1 * np.eye(n)
    c = rng.randn(T, B, n)
    K, k = 0.1 * rng.randn(T, B, nc, na), 0.3 * rng.randn(T, B, nc)

    def carry_step(z, u, net):
        return np.concatenate((np.asarray(u, dtype=np.float64), orig(np.asarray(z)[:, nc:], u, inner)), 1)
    orig = E.mlp_step
    E.mlp_step = carry_step
    try:
        zs = E.traj(E.MLP, z0, u0, aug)
        nx, nu, costs, full, alphas, trials, old = E.rollout_batched(E.MLP, aug, z0, C, c, K, k, zs, u0, -0.6, 0.6, 0.2, 5)
    finally:
        E.mlp_step = orig
    r = host_rollout(host, aug, z0, None, None, None, u0, None, None, None, None, None, 0.2, 1, True, carry=nc)
    close(r["new_x"], zs, "augmented trajectory")
    assert np.array_equal(r["new_x"][1:, :, :nc], u0[:-1])                       # the control itself, not a product with 1.0
    r = host_rollout(host, aug, z0, C, c, zs, u0, K, k, old, -0.6, 0.6, 0.2, 5, False, carry=nc)
    assert np.array_equal(r["alphas"], running(alphas, 0.2))
    close(r["new_x"], nx, "new_x")
    close(r["new_u"], nu, "new_u")
    np.testing.assert_allclose(r["costs"], costs, rtol=BAR)


def test_host_run_is_reproducible_and_handles_one_timestep(host):
    net = random_net(5, 2, [9], "elu", True, seed=3, scale=2.0)
    rng = np.random.RandomState(0)
    x0, u0 = rng.randn(2, 5), rng.randn(1, 2, 2)
    C = np.broadcast_to(np.eye(7), (1, 2, 7, 7)).copy()
    c = rng.randn(1, 2, 7)
    r = host_rollout(host, net, x0, C, c, None, u0, None, None, None, None, None, 0.2, 1, True)     # T = 1: no network call
    assert np.array_equal(r["new_x"][0], x0)
    np.testing.assert_allclose(r["costs"], E.quad_cost(C, c, x0[None], u0), rtol=BAR)
    x, u = rng.randn(7, 5), rng.randn(7, 2)
    a, b = host_linearize(host, net, x, u, True), host_linearize(host, net, x, u, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------
# (d) the same file, stand-alone, under the host sanitizers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_stand_alone_host_program_under_the_sanitizers(tmp_path, sanitizers):
    """tests/nn64_host.cpp with its own main.  AddressSanitizer + UndefinedBehaviorSanitizer: its LDS stand-in is a heap block
    of exactly the doubles the launch plan gives a wavefront, so an index past a kernel's area is an error here.
    ThreadSanitizer: the lanes are threads and `sync()` their only ordering, so an LDS value one lane writes and another reads
    without a `sync()` between them -- on the device, a store the compiler may move past the load -- is a reported race."""
    cxx = _cxx()
    if not cxx:
        pytest.skip("needs clang++")
    exe = str(tmp_path / "nn64_host")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function",
                            "-fsanitize=" + sanitizers, "-fno-sanitize-recover=undefined", "-DNN64_HOST_MAIN", "-I", CSRC, "-o", exe,
                            HOST_SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "nn64_host: ok" in run.stdout, run.stdout + run.stderr
