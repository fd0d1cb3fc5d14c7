"""MPC_KKT_MFMA40_NARROW16 / _NARROW4 on the device: the fused KKT backward of the padded 32/8 kernel on ONE 16-row state tile
(csrc/lqr_mfma40_body.h with -DMPC_MFMA40_XT=1 -DMPC_MFMA40_KKT, pass 2's workspace packed for it), asked for through
mpc_lqr_kkt_fused_kernel -- `plan_kkt_backward(kernel=...)`, `LQRStep(narrow_kkt_kernel=True)`, `mpc.MPC(narrow_kkt_kernel=True)`.

The problems are built in numpy, so the float64 oracle vouches for (x*, u*) and for the share of controls on a bound before the
device sees them.  Every case is held to the oracle by the method and number of
tests/test_gpu_fullsize.py::test_fused_kkt_backward_on_padded_mfma40_shapes_vs_oracle (3e-4 of each problem's scale) and to the padded
two-tile kernel on the same tensors, where equality is the expectation: the order of every sum over real terms is the same, the
second state tile holds exact zeros."""
import functools

import numpy as np
import pytest
import torch

from mpc import _native, mpc
from mpc._native import (KKT_MFMA40_NARROW4, KKT_MFMA40_NARROW16, KKT_MFMA40_PAD4, KKT_MFMA40_PAD16, KKT_NONE, KKT_PREFER_NARROW,
                         StepOptions)
from mpc.mpc import LinDx, QuadCost

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = ("dx_init", "dC", "dc", "dF", "df", "dx", "du")
SHAPES = [(13, 4, 12, 70), (16, 4, 12, 70), (16, 8, 12, 70), (9, 6, 12, 70), (14, 3, 12, 70), (16, 4, 2, 70), (16, 4, 1, 70), (16, 4, 12, 1),
          (5, 3, 12, 70)]


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()
    return _native.HipBackend()


def host(t):
    return t.detach().cpu().numpy()


def _shape_problem(rng, T, B, ns, nc, with_f=True):
    """tests/test_emu_mfma16.py's recipe, draw for draw"""
    n = ns + nc
    A = rng.standard_normal((T, B, n, n))
    C = np.einsum("tbji,tbjk->tbik", A, A) + 0.5 * np.eye(n)
    c = rng.standard_normal((T, B, n))
    F = np.concatenate((np.eye(ns) + 0.2 * rng.standard_normal((T - 1, B, ns, ns)) / np.sqrt(ns),
                        rng.standard_normal((T - 1, B, ns, nc)) / np.sqrt(ns)), 3)
    f = 0.1 * rng.standard_normal((T - 1, B, ns)) if with_f else None
    return dict(C=C, c=c, F=F, f=f, x_init=rng.standard_normal((B, ns)))


@functools.lru_cache(maxsize=None)
def reference(ns, nc, T, B, mode, with_f):
    """One problem per (shape, bounds, f), in float32-representable float64: inputs, (x*, u*) after four oracle steps under the
    bounds (unbounded: under +-0.4 too -- the backward needs a point, not an optimum), dl_dx, dl_du, the oracle's backward and the
    share of controls on a bound.  Computed once, never written to."""
    from oracle import lqr_oracle as O
    r32 = lambda a: None if a is None else np.asarray(a, np.float32).astype(np.float64)
    rng = np.random.default_rng(1900 + 100 * ns + nc + T + B)
    pr = {k: r32(v) for k, v in _shape_problem(rng, T, B, ns, nc, with_f=with_f).items()}
    cur_u = np.clip(0.5 * rng.standard_normal((T, B, nc)), -0.4, 0.4)
    cur_x, _ = O.traj_cost(pr["x_init"], cur_u, pr["F"], pr["f"])
    lo, hi = -0.4, 0.4
    if mode == "tensor":
        lo, hi = r32(-0.3 - 0.2 * rng.random((T, B, nc))), r32(0.3 + 0.2 * rng.random((T, B, nc)))
    x, u = cur_x, cur_u
    for _ in range(4):
        sol = O.lqr_step(lockstep=False, cur_x=x, cur_u=u, u_lower=lo, u_upper=hi, **pr)
        x, u = sol["new_x"], sol["new_u"]
    x, u = r32(x), r32(u)
    dl_dx, dl_du = r32(rng.standard_normal((T, B, ns))), r32(rng.standard_normal((T, B, nc)))
    blo, bhi = (None, None) if mode == "unbounded" else (lo, hi)
    o = O.kkt_backward(pr["C"], pr["c"], pr["F"], pr["f"], x, u, dl_dx, dl_du, blo, bhi, lockstep=False, nthreads=O.max_threads())
    share = float(((np.abs(u - lo) <= 1e-8) | (np.abs(u - hi) <= 1e-8)).mean())
    out = dict(pr, x=x, u=u, dl_dx=dl_dx, dl_du=dl_du, lo=blo, hi=bhi, oracle=o, share=share)
    for v in list(out.values()) + list(o.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def on_device(z, off_grid=False):
    """the problem's tensors on the device in float32; off_grid: C, c and F one float off the 16-byte grid"""
    def put(a, skew=False):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
        if skew:
            buf = torch.empty(t.numel() + 1, device=DEV, dtype=torch.float32)
            buf[1:].copy_(t.reshape(-1))
            t = buf[1:].view(t.shape)
            assert t.numel() == 0 or t.data_ptr() % 16 == 4
        return t
    d = {k: put(z[k], off_grid and k in ("C", "c", "F")) for k in ("C", "c", "F", "f", "x", "u", "dl_dx", "dl_du")}
    lo, hi = z["lo"], z["hi"]
    if isinstance(lo, np.ndarray):
        lo, hi = put(lo), put(hi)
    d["opts"] = StepOptions(u_lower=lo, u_upper=hi, c_symmetric=True)
    return d


def plan_for(be, d, **kw):
    plan = be.plan_kkt_backward(d["C"], d["c"], d["F"], d["f"], d["x"], d["u"], d["dl_dx"], d["dl_du"], d["opts"], **kw)
    assert plan is not None
    for k in GRADS:
        if plan.outputs[k] is not None:
            plan.outputs[k].fill_(float("nan"))
    return plan


def run(plan):
    got = plan()
    assert got is not None
    torch.cuda.synchronize()
    return got


def check_oracle(got, o, what):
    for k in GRADS:
        if o.get(k) is None or o[k].size == 0:
            assert got[k] is None or got[k].numel() == 0, k
            continue
        a = host(got[k]).astype(np.float64)
        assert np.isfinite(a).all(), (what, k)
        ax = tuple(i for i in range(a.ndim) if i != (0 if k == "dx_init" else 1))
        scale = np.maximum(1.0, np.abs(o[k]).max(axis=ax, keepdims=True))
        rel = (np.abs(a - o[k]) / scale).max(axis=ax)
        print("%s %s: worst problem %.2e of its scale" % (what, k, rel.max()))
        assert rel.max() < 3e-4, "%s %s: problem %d off by %.2e of its scale" % (what, k, int(rel.argmax()), rel.max())


def check_equal(got, want, what):
    for k in GRADS:
        if want[k] is None or want[k].numel() == 0:
            continue
        diff = float((got[k].double() - want[k].double()).abs().max())
        print("%s %s: max difference %.3e" % (what, k, diff))
        assert torch.equal(got[k], want[k]), "%s %s: differs from the two-tile kernel's by up to %.3e" % (what, k, diff)


@pytest.mark.parametrize("with_f", [True, False], ids=["f", "nof"])
@pytest.mark.parametrize("mode", ["unbounded", "scalar", "tensor"])
@pytest.mark.parametrize("ns,nc,T,B", SHAPES)
def test_narrow_fused_backward_against_the_oracle_and_the_padded_kernel(be, ns, nc, T, B, mode, with_f):
    z = reference(ns, nc, T, B, mode, with_f)
    if mode != "unbounded":
        print("share of controls on a bound: %.3f" % z["share"])
        assert 0.05 < z["share"] < 0.9, z["share"]
    d = on_device(z)
    by_code = (ns, nc) == (5, 3)          # up to 12/4 the family keeps the 12/4 kernels: the dword kernel by its code, against the padded by its
    sixteen = ns % 4 == 0 and nc % 4 == 0
    plan = plan_for(be, d, kernel=KKT_MFMA40_NARROW4 if by_code else KKT_PREFER_NARROW)
    want = KKT_MFMA40_NARROW4 if by_code or not sixteen else KKT_MFMA40_NARROW16
    assert plan.kernel == want and be.kkt_route(plan) == want
    wide = plan_for(be, d, kernel=KKT_MFMA40_PAD4) if by_code else plan_for(be, d)
    assert wide.kernel == (KKT_MFMA40_PAD16 if sixteen and not by_code else KKT_MFMA40_PAD4) == be.kkt_route(wide)
    got, ref = run(plan), run(wide)
    check_oracle(got, z["oracle"], "narrow")
    check_oracle(ref, z["oracle"], "padded")
    check_equal(got, ref, "narrow")


def test_caller_kept_dx_du_or_the_workspaces_and_two_runs(be):
    z = reference(16, 4, 12, 70, "scalar", True)
    d = on_device(z)
    plan = plan_for(be, d, kernel=KKT_PREFER_NARROW)
    first = {k: run(plan)[k].clone() for k in GRADS}
    for k in GRADS:
        plan.outputs[k].fill_(float("nan"))
    again = run(plan)
    for k in GRADS:
        assert torch.equal(first[k], again[k]), k
    # the same call with dx_out = du_out = NULL: the kernel keeps dx, du in its workspace (the last 24 of its 448 floats a problem-step)
    other = plan_for(be, d, kernel=KKT_PREFER_NARROW)
    args = list(other._bind)
    assert args[10] == other.outputs["dx"].data_ptr() and args[11] == other.outputs["du"].data_ptr()
    args[10] = args[11] = None
    assert int(_native.load().mpc_lqr_kkt_fused_kernel_route(*args)) == KKT_MFMA40_NARROW16
    rc = _native.load().mpc_lqr_kkt_fused_kernel(*args, torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k in ("dx_init", "dC", "dc", "dF", "df"):
        assert torch.equal(other.outputs[k], first[k]), k


def test_blocks_off_the_16_byte_grid_take_the_dword_kernel_and_give_the_same_numbers(be):
    z = reference(16, 4, 12, 70, "scalar", True)
    on_grid = plan_for(be, on_device(z), kernel=KKT_PREFER_NARROW)
    off_grid = plan_for(be, on_device(z, off_grid=True), kernel=KKT_PREFER_NARROW)
    assert on_grid.kernel == KKT_MFMA40_NARROW16 and off_grid.kernel == KKT_MFMA40_NARROW4 == be.kkt_route(off_grid)
    a, b = run(on_grid), run(off_grid)
    check_oracle(b, z["oracle"], "off the grid")
    check_equal(b, a, "off the grid")


def test_an_exact_code_that_does_not_fit_raises_and_launches_nothing(be):
    d = on_device(reference(13, 4, 12, 70, "scalar", True))
    with pytest.raises(RuntimeError, match="MPC_KKT_MFMA40_NARROW16 needs n_state <= 16, n_ctrl <= 8, both multiples of 4"):
        plan_for(be, d, kernel=KKT_MFMA40_NARROW16)


# ---------------------------------------------------------------------------------------------
# end to end: mpc.MPC(narrow_kkt_kernel=True)
# ---------------------------------------------------------------------------------------------
def _solve(monkeypatch, ns, nc, flag, slew=False, box=True, asym=False, T=8, B=6):
    kernels = []
    orig = _native.HipBackend.plan_kkt_backward

    def spy(self, *a, **k):
        plan = orig(self, *a, **k)
        kernels.append(None if plan is None else (plan.kernel, _native.HipBackend.kkt_route(plan)))
        return plan
    monkeypatch.setattr(_native.HipBackend, "plan_kkt_backward", spy)
    g = torch.Generator().manual_seed(43)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    n = ns + nc
    L = r(T, B, n, n)
    C = (L @ L.transpose(-1, -2) / n + torch.eye(n, dtype=torch.float64)).float().to(DEV)
    if asym:                             # one C_t of one problem is not symmetric
        C[2, 4, 1, n - 1] += 0.5
    c = r(T, B, n).float().to(DEV)
    F = (0.2 * r(T - 1, B, ns, n) + torch.cat((torch.eye(ns, dtype=torch.float64), torch.zeros(ns, nc, dtype=torch.float64)), 1)).float().to(DEV)
    f = (0.1 * r(T - 1, B, ns)).float().to(DEV)
    x0 = r(B, ns).float().to(DEV)
    leaves = [t.requires_grad_(True) for t in (C, c, F, f)]
    extra = dict(slew_rate_penalty=1.0) if slew else {}
    bounds = dict(u_lower=-0.3, u_upper=0.3) if box else {}
    ctrl = mpc.MPC(ns, nc, T, lqr_iter=8, verbose=-1, exit_unconverged=False, detach_unconverged=False, n_batch=B,
                   **bounds, **extra, **(dict(narrow_kkt_kernel=True) if flag else {}))
    x, u, _ = ctrl(x0, QuadCost(leaves[0], leaves[1]), LinDx(leaves[2], leaves[3]))
    w = torch.Generator().manual_seed(44)
    loss = (x * torch.randn(x.shape, generator=w).to(DEV)).sum() + (u * torch.randn(u.shape, generator=w).to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(_native.HipBackend, "plan_kkt_backward", orig)
    grads = [t.grad for t in leaves]
    assert all(gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0 for gr in grads)
    if box:
        assert int((u.detach().abs() == 0.3).sum()) > 0
    return grads, kernels


def test_mpc_13_4_with_the_flag_differentiates_on_the_narrow_kernel_and_equals_the_flag_off_solve(be, monkeypatch):
    on, k_on = _solve(monkeypatch, 13, 4, True)
    off, k_off = _solve(monkeypatch, 13, 4, False)
    assert k_on == [(KKT_MFMA40_NARROW4,) * 2] and k_off == [(KKT_MFMA40_PAD4,) * 2], (k_on, k_off)
    for name, a, b in zip("CcFf", on, off):
        assert torch.equal(a, b), "d%s differs by up to %.3e" % (name, float((a - b).abs().max()))


@pytest.mark.parametrize("box", [False, True], ids=["unbounded", "box"])
def test_mpc_12_4_slew_with_the_flag_differentiates_at_16_4_on_the_narrow_kernel(be, monkeypatch, box):
    """flag off, the slew ending makes no symmetry promise and its backward is the three-call route (prepare, nested step, closed
    form): other kernels, so the two are held together by the float64-oracle tolerance of
    tests/test_gpu_parity.py::test_kkt_backward_wave_kernels, 2e-4 of the largest entry."""
    on, k_on = _solve(monkeypatch, 12, 4, True, slew=True, box=box)
    off, k_off = _solve(monkeypatch, 12, 4, False, slew=True, box=box)
    assert k_on == [(KKT_MFMA40_NARROW16,) * 2], k_on
    assert k_off == [None], k_off                          # no promise: mpc_lqr_kkt_fused_supported says no, no plan is bound
    for name, a, b in zip("CcFf", on, off):
        scale = max(1.0, float(b.abs().max()))
        diff = float((a - b).abs().max()) / scale
        print("d%s: %.3e of the largest entry" % (name, diff))
        assert diff < 2e-4, "d%s: %.3e of the largest entry" % (name, diff)


def test_mpc_12_4_slew_with_a_nonsymmetric_C_makes_no_promise_and_equals_the_flag_off_solve(be, monkeypatch):
    on, k_on = _solve(monkeypatch, 12, 4, True, slew=True, asym=True)
    off, k_off = _solve(monkeypatch, 12, 4, False, slew=True, asym=True)
    assert all(k is None or k == (KKT_NONE, KKT_NONE) for k in k_on) and k_on == k_off, (k_on, k_off)
    for name, a, b in zip("CcFf", on, off):
        assert torch.equal(a, b), "d%s differs by up to %.3e" % (name, float((a - b).abs().max()))
