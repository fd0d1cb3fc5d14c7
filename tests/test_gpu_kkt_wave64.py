"""The float64 wavefront kernels of the KKT backward's closed-form part (csrc/kkt_wave64.hip, mpc_lqr_kkt_grads_kernel with
MPC_KKT_GRADS_WAVE64; docs/history/r27.md) on the MI355X.

Problems are built as tests/test_gpu_generic.py::test_kkt_backward_through_the_generic_gradient_kernel builds them: C = A'A / n +
0.1 I, random F (and f), random cotangents, x*, u* from the kernel's own step; with bounds +-0.5 some controls sit exactly on a
bound and some are free (asserted here on the kernel's step, and from the oracle alone in a test without the gpu mark).

  1. the whole backward, be.kkt_backward(..., grads_kernel=KKT_GRADS_WAVE64), against oracle.lqr_oracle.kkt_backward in float64:
     |err| <= 1e-9 max(1, max |oracle|) for every one of dx_init, dC, dc, dF, df -- the project's float64 limit.
  2. the gradient call alone into NaN-filled buffers, against mpc_lqr_kkt_grads (the generic kernel) on the same dx, du: dc bitwise;
     dC within 4 * 2^-53 (|dtau_i tau_j| + |tau_i dtau_j|) per element -- two roundings on each side, whichever side contracts to an
     fma; dF, df, dx_init pass through recursions summed in another order and are held to the oracle under 1.
  3. a C that is not symmetric: the same limit (the recursion reads rows of C as given).
  4. views: stride-0 expands over the batch and a C moved off the 16-byte grid, bitwise the contiguous / unshifted call (the general
     form's arithmetic order is the aligned form's by design).
  5. two calls are bitwise equal.   6. the route queries.   7. mpc.MPC(f64_grad_kernel=True) end to end.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
GRAD_KEYS = ("dx_init", "dC", "dc", "dF", "df")
F64_LIMIT = 1e-9

# (n_state, n_ctrl, T, B): the smallest at which each piece can go wrong
SHAPES = [(1, 1, 3, 2),        # n = 2: the parking needs 2 n_state doubles of dF_t
          (2, 1, 4, 3),        # odd n
          (7, 3, 5, 3),        # n even, n_state odd: the general form
          (12, 4, 7, 9),       # the aligned form
          (12, 4, 2, 3),       # a ring deeper than the horizon
          (12, 4, 1, 2),       # T = 1: no F, no dF
          (13, 4, 1, 2),
          (13, 4, 6, 3),       # odd n_state with a larger n
          (32, 8, 9, 5),       # blocks of many DMA instructions
          (60, 4, 3, 2),       # n = 64, LDS above 64 KiB
          (63, 1, 2, 2)]       # the largest general-form stage: the vmcnt(0) ring
CASES = [shape + (with_f, bounded) for shape in SHAPES for with_f in (True, False) for bounded in (False, True)]
ASYM_CASES = [(12, 4, 7, 9, True, True), (13, 4, 6, 3, True, True)]
# four controls in all at 63/1: these seeds leave some of them inside the box (the oracle-only test below holds every recipe to that)
SALT = {(63, 1, 2, 2, True): 100084, (63, 1, 2, 2, False): 100000}


def case_id(case):
    ns, nc, T, B, with_f, bounded = case[:6]
    return "%d/%d-T%d-B%d%s%s" % (ns, nc, T, B, "-f" if with_f else "", "-box" if bounded else "")


def O():
    from oracle import lqr_oracle
    return lqr_oracle


@functools.lru_cache(maxsize=None)
def problem(ns, nc, T, B, with_f, bounded, asym=False):
    """The float64 arrays of one case (never changed afterwards): x_init, C, c, F, f, the nominal (cur_x on the dynamics), the
    cotangents gx, gu and the bounds.  asym: C + 0.05 (a random antisymmetric matrix) on two of the problems."""
    n = ns + nc
    rng = np.random.default_rng(27000 + 1000 * ns + 100 * nc + 10 * T + 2 * with_f + bounded + 5 * asym +
                                SALT.get((ns, nc, T, B, with_f), 0) * bounded)
    A = rng.standard_normal((T, B, n, n))
    C = np.einsum("tbji,tbjk->tbik", A, A) / n + 0.1 * np.eye(n)
    if asym:
        S = rng.standard_normal((T, 2, n, n))
        C[:, :2] += 0.05 * (S - S.transpose(0, 1, 3, 2))
    F = np.concatenate((np.eye(ns) + 0.2 * rng.standard_normal((max(T - 1, 0), B, ns, ns)) / np.sqrt(ns),
                        rng.standard_normal((max(T - 1, 0), B, ns, nc)) / np.sqrt(ns)), 3)
    f = 0.1 * rng.standard_normal((max(T - 1, 0), B, ns)) if with_f else None
    cur_u = 0.3 * rng.standard_normal((T, B, nc))
    if bounded:
        cur_u = np.clip(cur_u, -0.5, 0.5)
    x_init = rng.standard_normal((B, ns))
    cur_x = O().traj_cost(x_init, cur_u, F, f)[0]
    lo, hi = (-0.5, 0.5) if bounded else (None, None)
    return dict(x_init=x_init, C=C, c=rng.standard_normal((T, B, n)), F=F, f=f, cur_x=cur_x, cur_u=cur_u,
                gx=rng.standard_normal((T, B, ns)), gu=rng.standard_normal((T, B, nc)), lo=lo, hi=hi)


@pytest.mark.parametrize("case", [c for c in CASES if c[5]] + ASYM_CASES, ids=case_id)
def test_the_bounded_recipes_pin_some_controls_and_free_others(case):
    """From the oracle alone: its step from the case's nominal ends with controls on a bound and controls inside."""
    p = problem(*case, asym=case in ASYM_CASES)
    r = O().lqr_step(p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"], p["lo"], p["hi"])
    act = np.abs(r["new_u"]) == 0.5
    assert 0 < act.sum() < act.size, act.mean()


# ---------------------------------------------------------------------------------------------
# on the device
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mpc import _native
    b = _native.HipBackend()
    _native.load()            # fail loudly if the extension is missing
    return b


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def options(p):
    from mpc._native import StepOptions
    return StepOptions(u_lower=p["lo"], u_upper=p["hi"])


_SOLVED = {}


def solved(be, case, asym=False):
    """One case on the device, computed once and shared: the tensors, x*, u* of the kernel's own step, the oracle's backward at
    them, and the whole backward through the float64 wavefront kernels (with the nested solve's dx, du)."""
    key = case + (asym,)
    if key not in _SOLVED:
        from mpc._native import KKT_GRADS_WAVE64
        p = problem(*case, asym=asym)
        d = {k: dev(p[k]) for k in ("x_init", "C", "c", "F", "f", "cur_x", "cur_u", "gx", "gu")}
        r = be.lqr_step(d["x_init"], d["C"], d["c"], d["F"], d["f"], d["cur_x"], d["cur_u"], options(p))
        torch.cuda.synchronize()
        xs, us = host(r["new_x"]), host(r["new_u"])
        if p["lo"] is not None:
            act = np.abs(us) == 0.5
            assert 0 < act.sum() < act.size, act.mean()           # some controls pinned, some free
        o64 = O().kkt_backward(p["C"], p["c"], p["F"], p["f"], xs, us, p["gx"], p["gu"], p["lo"], p["hi"], lockstep=False)
        g = be.kkt_backward(d["C"], d["c"], d["F"], d["f"], r["new_x"], r["new_u"], d["gx"], d["gu"], options(p),
                            grads_kernel=KKT_GRADS_WAVE64)
        torch.cuda.synchronize()
        _SOLVED[key] = dict(p=p, d=d, xs=r["new_x"], us=r["new_u"], o64=o64, g=g)
    return _SOLVED[key]


def hold_to_the_oracle(label, g, o64):
    worst = {}
    for k in GRAD_KEYS:
        if o64[k] is None or o64[k].size == 0:
            assert g[k] is None or g[k].numel() == 0, k
            continue
        assert g[k] is not None, k
        a = host(g[k])
        assert np.isfinite(a).all(), k
        worst[k] = float(np.abs(a - o64[k]).max() / (F64_LIMIT * max(1.0, np.abs(o64[k]).max())))
    print("[wave64] %s: worst err/limit %.3g  (%s)" % (label, max(worst.values()), " ".join("%s %.2g" % kv for kv in worst.items())))
    for k, w in worst.items():
        assert w <= 1.0, "%s %s: %.3g of the limit" % (label, k, w)


def grads_alone(be, s, kernel, C=None, c=None, F=None):
    """mpc_lqr_kkt_grads_kernel (kernel = 0: mpc_lqr_kkt_grads) alone on the nested solve's dx, du of case `s`, into buffers full of
    NaN; C, c, F: views to hand over instead of the case's tensors.  -> (outputs, the two route queries' answers)"""
    from mpc import _native
    d, g = s["d"], s["g"]
    C, c, F = (d["C"] if C is None else C), (d["c"] if c is None else c), (d["F"] if F is None else F)
    B, ns = d["x_init"].shape
    prob, keepalive = be._problem(torch.zeros(B, ns, dtype=torch.float64, device=DEV), C, c, F, d["f"], s["xs"], s["us"])
    out = {k: None if g[k] is None else torch.full_like(g[k], float("nan")) for k in GRAD_KEYS}
    ptr = lambda t: None if t is None else t.data_ptr()
    args = (g["dx"].data_ptr(), g["du"].data_ptr(), d["gx"].data_ptr(), d["gu"].data_ptr(), ptr(out["dC"]), ptr(out["dc"]),
            ptr(out["dF"]) if out["dF"].numel() else None, ptr(out["df"]), ptr(out["dx_init"]))
    L = _native.load()
    routes = (int(L.mpc_lqr_kkt_grads_kernel_route(ctypes.byref(prob), _native.KKT_GRADS_WAVE64, *args)),
              int(L.mpc_lqr_kkt_grads_route(ctypes.byref(prob), *args)))
    stream = torch.cuda.current_stream().cuda_stream
    if kernel:
        rc = L.mpc_lqr_kkt_grads_kernel(ctypes.byref(prob), kernel, *args, stream)
    else:
        rc = L.mpc_lqr_kkt_grads(ctypes.byref(prob), *args, stream)
    torch.cuda.synchronize()
    assert rc == 0, L.mpc_lqr_last_error().decode()
    del keepalive
    return out, routes


def every_entry_written(out):
    for k in GRAD_KEYS:
        if out[k] is not None:
            assert bool(torch.isfinite(out[k]).all()), k


def bitwise(a, b, what):
    for k in GRAD_KEYS:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), "%s: %s differs by up to %.3e" % (what, k, float((a[k] - b[k]).abs().max()))


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_backward_against_the_oracle_and_the_generic_kernel(be, case):
    from mpc._native import KKT_GRADS_GENERIC, KKT_GRADS_WAVE64
    ns, nc, T, B, with_f, bounded = case
    s = solved(be, case)
    g, o64 = s["g"], s["o64"]
    # 1. the whole backward against the oracle
    assert (g["df"] is None) == (o64["df"] is None) == (not with_f or T == 1)
    hold_to_the_oracle(case_id(case), g, o64)
    # 2. the gradient call alone: every entry written; dc bitwise and dC within two roundings of the generic kernel's
    wave, routes = grads_alone(be, s, KKT_GRADS_WAVE64)
    every_entry_written(wave)
    generic, _ = grads_alone(be, s, 0)
    every_entry_written(generic)
    assert torch.equal(wave["dc"], generic["dc"])
    tau = np.concatenate((host(s["xs"]), host(s["us"])), 2)
    dtau = np.concatenate((host(g["dx"]), host(g["du"])), 2)
    bound = 4 * 2.0 ** -53 * (np.abs(dtau[..., :, None] * tau[..., None, :]) + np.abs(tau[..., :, None] * dtau[..., None, :]))
    err = np.abs(host(wave["dC"]) - host(generic["dC"]))
    assert (err <= bound).all(), "dC: %.3g of the bound" % float((err / np.maximum(bound, 1e-300)).max())
    # (the alone call is the whole backward's closed-form part: the same bits)
    bitwise(wave, g, "alone against the whole backward")
    # 5. two calls are bitwise equal
    again, _ = grads_alone(be, s, KKT_GRADS_WAVE64)
    bitwise(again, wave, "second call")
    # 6. the routes on the very tensors
    assert routes == (KKT_GRADS_WAVE64, KKT_GRADS_GENERIC)


@gpu
@pytest.mark.parametrize("case", ASYM_CASES, ids=case_id)
def test_a_c_that_is_not_symmetric_is_read_by_rows(be, case):
    """3. C + 0.05 (antisymmetric) on two problems: a column read of C would miss the oracle here by far more than the limit."""
    s = solved(be, case, asym=True)
    C = s["p"]["C"]
    assert np.abs(C[:, :2] - C[:, :2].transpose(0, 1, 3, 2)).max() > 0.05 and np.array_equal(C[:, 2:], C[:, 2:].transpose(0, 1, 3, 2))
    hold_to_the_oracle(case_id(case) + " asym", s["g"], s["o64"])


@gpu
@pytest.mark.parametrize("case", [(12, 4, 7, 9, True, True), (13, 4, 6, 3, True, False)], ids=case_id)
def test_views_give_the_bits_of_their_contiguous_copies(be, case):
    """4. C, c, F as stride-0 expands over the batch; C's storage moved by one double (on 8 bytes, not on 16: the general form)."""
    from mpc._native import KKT_GRADS_WAVE64
    s = solved(be, case)
    d = s["d"]
    B = d["C"].shape[1]
    shared = [t[:, :1].contiguous().expand(-1, B, *t.shape[2:]) for t in (d["C"], d["c"], d["F"])]
    assert all(t.stride(1) == 0 for t in shared)
    on_views, routes = grads_alone(be, s, KKT_GRADS_WAVE64, *shared)
    on_copies, _ = grads_alone(be, s, KKT_GRADS_WAVE64, *(t.contiguous() for t in shared))
    every_entry_written(on_views)
    assert routes[0] == KKT_GRADS_WAVE64
    bitwise(on_views, on_copies, "stride-0 views")
    # the shifted C
    room = torch.empty(d["C"].numel() + 1, dtype=torch.float64, device=DEV)
    assert room.data_ptr() % 16 == 0
    moved = room[1:].view_as(d["C"])
    moved.copy_(d["C"])
    assert moved.data_ptr() % 16 == 8
    on_moved, routes = grads_alone(be, s, KKT_GRADS_WAVE64, C=moved)
    unmoved, _ = grads_alone(be, s, KKT_GRADS_WAVE64)
    every_entry_written(on_moved)
    assert routes[0] == KKT_GRADS_WAVE64
    bitwise(on_moved, unmoved, "C moved by one double")


@gpu
def test_mpc_with_the_flag_differentiates_through_the_float64_wavefront_kernels(be, monkeypatch):
    """7. 12/4, T = 5, B = 3, box +-0.5: the gradients of a random linear functional of (x, u) with respect to C, c, F, x_init,
    flag on against flag off, within 1e-9 max(1, max |.|)."""
    from mpc import _native, mpc
    from mpc.mpc import LinDx, QuadCost
    ns, nc, T, B = 12, 4, 5, 3
    p = problem(ns, nc, T, B, True, True)
    asked = []
    orig = _native.HipBackend.kkt_backward

    def spy(self, *a, **k):
        asked.append(k.get("grads_kernel", 0))
        return orig(self, *a, **k)
    monkeypatch.setattr(_native.HipBackend, "kkt_backward", spy)

    def solve(flag):
        leaves = [dev(p[k]).requires_grad_(True) for k in ("C", "c", "F", "x_init")]
        ctrl = mpc.MPC(ns, nc, T, u_lower=-0.5, u_upper=0.5, lqr_iter=8, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                       n_batch=B, **(dict(f64_grad_kernel=True) if flag else {}))
        x, u, _ = ctrl(leaves[3], QuadCost(leaves[0], leaves[1]), LinDx(leaves[2], dev(p["f"])))
        w = torch.Generator().manual_seed(45)
        wx, wu = torch.randn(x.shape, generator=w, dtype=torch.float64).to(DEV), torch.randn(u.shape, generator=w, dtype=torch.float64).to(DEV)
        ((x * wx).sum() + (u * wu).sum()).backward()
        torch.cuda.synchronize()
        act = u.detach().abs() == 0.5
        assert 0 < int(act.sum()) < act.numel()
        return [t.grad for t in leaves]
    on, off = solve(True), solve(False)
    assert asked == [_native.KKT_GRADS_WAVE64, 0], asked
    for name, a, b in zip(("C", "c", "F", "x_init"), on, off):
        assert a is not None and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        limit = F64_LIMIT * max(1.0, float(b.abs().max()))
        diff = float((a - b).abs().max())
        print("[wave64] mpc d%s: %.3g of the limit" % (name, diff / limit))
        assert diff <= limit, "d%s: %.3g of the limit" % (name, diff / limit)
