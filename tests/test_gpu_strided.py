"""GPU (-m gpu): every LQR kernel on strided C, c, F, f (and qp_start) views against the dense copy of the same values and the
oracle.  tests/strided_views.py carves each tensor out of its own NaN-filled arena through its own (st, sb) pair; the views go
through be.plan_step / be.lqr_step / be.kkt_backward / be.traj_cost as they are (mpc._native._problem must not copy them).

Per step case (a forced impl, a fixture, a layout the kernel's rule in csrc/lqr_rules.hip admits):
  1. every output -- pre-filled with NaN, the integer words with -1, on both sides -- is BITWISE the same forced impl's on the dense
     copy; K, k too (a second call with out->K / out->k);
  2. the oracle comparison of tests/test_gpu_parity.py: check_step where the case is a whole fixture shown as it is, its
     oracle lines (the same tolerances: 1e-9 in float64, rtol 1e-3 / atol 1e-4 in float32) where the layout shows a broadcast block
     or the fixture is cut to its first timesteps (nominal re-derived by O.traj_cost);
  3. a layout the rule does not admit is refused with MPC_E_DIMS before any launch;
  4. mpc_lqr_step_route names the kernel the case is named for.
tests/test_emu_strided.py runs the same layouts through the kernel sources on the CPU first."""
import ctypes

import numpy as np
import pytest
import torch

import strided_views as SV
from conftest import golden
from test_gpu_parity import DEV, be, check_step, dev, host  # noqa: F401  (be: the module-scoped backend fixture)

pytestmark = pytest.mark.gpu

E_DIMS = -1
STEP_OUT = ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alpha_du_norm", "alphas", "qp_iters", "status")
SHARED = ("shared", "shared_b", "shared_t")


def whole(name):
    from helpers import step_kwargs
    z = golden(name)
    return step_kwargs(z), z


def cut(name, T, B=None):
    return SV.cut(golden(name), T, B), None


def rand(ns, nc, T, B, seed, bounds=None, dtype=np.float32):
    return SV.random_case(ns, nc, T, B, seed, bounds=bounds, dtype=dtype), None


def symmetric(name, T):
    """The problems of an asym_* fixture whose C IS symmetric, cut to T timesteps: a regular fixture of that shape."""
    from helpers import asymmetric_problems, step_kwargs
    z = golden(name)
    keep = ~asymmetric_problems(z)
    kw = step_kwargs(z)
    for k, v in list(kw.items()):
        if isinstance(v, np.ndarray) and v.ndim >= 2 and k != "x_init":
            kw[k] = v[:, keep]
    kw["x_init"] = kw["x_init"][keep]
    zz = {"C": kw["C"], "c": kw["c"], "F": kw["F"], "f": kw["f"], "x_init": kw["x_init"], "cur_x": kw["cur_x"], "cur_u": kw["cur_u"],
          "delta_u": z["delta_u"], "decay": z["decay"], "meta": z["meta"]}
    return SV.cut(zz, T), None


# id -> (impl, builder, layouts, qp_start hint, environment)
I_GEN, I_MFMA16, I_DPP16, I_TINY, I_MFMA40, I_WAVE1, I_PAD40, I_PAD12, I_NARROW = 1, 2, 3, 4, 5, 6, 7, 8, 9
ALL, GRID = SV.LAYOUTS, SV.GRID
STEP = {
    "3-masked-resident0": (I_DPP16, lambda: whole("step_masked_nc4_f32"), ALL, False, {"MPC_DPP16_RESIDENT": "0"}),
    "3-unbounded-resident1": (I_DPP16, lambda: cut("step_ns_unbounded_f32", 9), ALL, False, {"MPC_DPP16_RESIDENT": "1"}),
    "3-unbounded-resident0": (I_DPP16, lambda: cut("step_ns_unbounded_f32", 9), ALL, False, {"MPC_DPP16_RESIDENT": "0"}),
    "3-box-hint": (I_DPP16, lambda: cut("step_ns_bounded_f32", 9), ALL, True, {}),
    "8-7_3": (I_PAD12, lambda: symmetric("step_asym_odd_f32", 9), ALL, False, {}),
    "8-8_4-box": (I_PAD12, lambda: rand(8, 4, 6, 5, 84, bounds=0.4), ALL, True, {}),
    "8-12_4-off-the-grid": (I_PAD12, lambda: cut("step_ns_bounded_f32", 6), ("pitch_off", "mixed_a"), False, {}),
    "2-cfg1-f32": (I_MFMA16, lambda: whole("step_cfg1_f32"), ALL, False, {}),
    "2-cfg1-f64": (I_MFMA16, lambda: whole("step_cfg1_f64"), ALL, False, {}),
    "2-ns-bounded-f64": (I_MFMA16, lambda: cut("step_ns_bounded_f64", 7), ALL, False, {}),
    "5-cfg5": (I_MFMA40, lambda: whole("step_cfg5_f32"), ALL, False, {}),
    "5-box-hint": (I_MFMA40, lambda: rand(32, 8, 6, 3, 328, bounds=0.4), ALL, True, {}),
    "7-13_4": (I_PAD40, lambda: rand(13, 4, 6, 3, 134), ALL, False, {}),
    "7-24_8": (I_PAD40, lambda: rand(24, 8, 6, 3, 248), ALL, False, {}),
    "7-20_4-box-hint": (I_PAD40, lambda: rand(20, 4, 6, 3, 204, bounds=0.4), ALL, True, {}),
    "9-13_4": (I_NARROW, lambda: rand(13, 4, 6, 3, 134), ALL, False, {}),
    "9-16_4-box-hint": (I_NARROW, lambda: rand(16, 4, 6, 3, 164, bounds=0.4), ALL, True, {}),
    "4-nc1-unbounded": (I_TINY, lambda: cut("step_nc1_unbounded_f32", 9), ALL, False, {}),
    "4-nc1-bounded": (I_TINY, lambda: cut("step_nc1_bounded_f32", 9), ALL, False, {}),
    "4-nc1-scalar-f64": (I_TINY, lambda: cut("step_nc1_scalar_f64", 9), ALL, False, {}),
    "6-nc1-unbounded": (I_WAVE1, lambda: cut("step_nc1_unbounded_f32", 9), ALL, False, {}),
    "6-nc1-bounded": (I_WAVE1, lambda: cut("step_nc1_bounded_f32", 9), ALL, False, {}),
    "1-cfg1-f64": (I_GEN, lambda: whole("step_cfg1_f64"), ALL, False, {}),
    "1-delta-f64": (I_GEN, lambda: whole("step_delta_f64"), ALL, False, {}),
    "1-nof-f64": (I_GEN, lambda: whole("step_unbounded_nof_f64"), ALL, False, {}),
    "1-cfg5-bounded-f64": (I_GEN, lambda: whole("step_cfg5_bounded_f64"), ALL, False, {}),
    "1-40_4-f32": (I_GEN, lambda: rand(40, 4, 5, 3, 404), ALL, False, {}),
    # impl 0: one case per family; the route must name a kernel whose rule admits the layout
    "0-12_4": (0, lambda: cut("step_ns_bounded_f32", 6), ("mixed_a", "pitch_off"), False, {}),
    "0-32_8": (0, lambda: whole("step_cfg5_f32"), ("mixed_a", "pitch_off"), False, {}),
    "0-16_4": (0, lambda: rand(16, 4, 6, 3, 164), ("mixed_a", "pitch_off"), False, {}),
    "0-7_3": (0, lambda: symmetric("step_asym_odd_f32", 9), ("mixed_a", "pitch_off"), False, {}),
    "0-5_1": (0, lambda: cut("step_nc1_bounded_f32", 9), ("mixed_a", "pitch_off"), False, {}),
    "0-4_2-f64": (0, lambda: whole("step_cfg1_f64"), ("mixed_a", "pitch_off"), False, {}),
}
AUTO_ROUTE = {"0-12_4": {"mixed_a": (I_DPP16,), "pitch_off": (I_PAD12,)}, "0-32_8": {"mixed_a": (I_MFMA40,), "pitch_off": (I_PAD40,)},
              "0-16_4": {"mixed_a": (I_PAD40,), "pitch_off": (I_PAD40,)}, "0-7_3": {"mixed_a": (I_PAD12,), "pitch_off": (I_PAD12,)},
              "0-5_1": {"mixed_a": (I_TINY, I_WAVE1), "pitch_off": (I_TINY, I_WAVE1)}, "0-4_2-f64": {"mixed_a": (I_MFMA16,), "pitch_off": (I_MFMA16,)}}
STEP_PARAMS = [(cid, layout) for cid, case in STEP.items() for layout in case[2]]
_BUILT = {}


def built(cid):
    if cid not in _BUILT:
        _BUILT[cid] = STEP[cid][1]()
    return _BUILT[cid]


def options(d, qp=None):
    from mpc._native import StepOptions
    lo, hi = d.get("u_lower"), d.get("u_upper")
    lo = dev(lo) if isinstance(lo, np.ndarray) else lo
    hi = dev(hi) if isinstance(hi, np.ndarray) else hi
    return StepOptions(u_lower=lo, u_upper=hi, u_zero_I=dev(d.get("u_zero_I")), delta_u=d.get("delta_u"),
                       linesearch_decay=d.get("linesearch_decay", 0.2), max_linesearch_iter=d.get("max_linesearch_iter", 10), qp_start=qp)


def admitted(impl, pl):
    """csrc/lqr_rules.hip, as tests/test_stride_rules_host.py holds it: the exact 12/4 and 32/8 kernels want the first block and both
    strides of C, c, F, f on 16 bytes; every other kernel takes any view."""
    if impl not in (I_DPP16, I_MFMA40):
        return True
    return SV.on_grid({r: pl[r] for r in ("C", "c", "F", "f")}, 4)


def tensors(d, layout, qp):
    """(placed views, the tensors of the view call, the tensors of the dense call)"""
    pl = SV.place_problem(layout, torch, d["C"], d["c"], d["F"], d.get("f"), qp, device=DEV)
    fixed = (dev(d["x_init"]),), (dev(d["cur_x"]), dev(d["cur_u"]))
    views = fixed[0] + tuple(None if pl[r] is None else pl[r].view for r in "CcFf") + fixed[1]
    dense = fixed[0] + tuple(None if pl[r] is None else pl[r].dense for r in "CcFf") + fixed[1]
    return pl, views, dense


def run_plan(be, args, opts, impl):
    plan = be.plan_step(*args, opts, impl=impl)
    for k, v in plan.outputs.items():
        v.fill_(-1 if v.dtype == torch.int32 else float("nan"))
    return plan


def not_copied(be, views, pl):
    p, _keep = be._problem(*views)
    for role in "CcFf":
        if pl[role] is not None:
            assert getattr(p, role) == pl[role].view.data_ptr()
            assert (getattr(p, role + "_st"), getattr(p, role + "_sb")) == (pl[role].st, pl[role].sb) == pl[role].view.stride()[:2]


def oracle(d):
    from oracle import lqr_oracle as O
    return O.lqr_step(lockstep=False, **{k: (SV.f64(v) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in d.items()})


def hold(r, o, f64):
    """check_step's comparisons with the oracle (tests/test_gpu_parity.py), for values no fixture holds the reference's outputs of."""
    if f64:
        for k in ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alphas"):
            np.testing.assert_allclose(r[k], o[k], err_msg=k, rtol=1e-9, atol=1e-9)
    else:
        np.testing.assert_allclose(r["new_x"], o["new_x"], rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(r["new_u"], o["new_u"], rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(r["alphas"], o["alphas"], rtol=1e-6)
    assert (r["status"] & 2 == 0).all()


@pytest.mark.parametrize("cid,layout", STEP_PARAMS, ids=["%s-%s" % p for p in STEP_PARAMS])
def test_step_on_views(be, cid, layout, monkeypatch):
    from mpc import _native
    impl, _builder, _layouts, hint, env = STEP[cid]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw, z = built(cid)
    d = SV.shown(kw, layout)
    f64 = d["C"].dtype == np.float64
    qp = None
    if hint:
        qp = np.random.default_rng(5).uniform(-0.4, 0.4, d["cur_u"].shape).astype(np.float32)
    pl, views, dense = tensors(d, layout, qp)
    not_copied(be, views, pl)
    opts_v, opts_d = options(d, None if qp is None else pl["qp_start"].view), options(d, None if qp is None else pl["qp_start"].dense)
    plan = run_plan(be, views, opts_v, impl)
    p, o_, out, _keep, ws = plan._keep
    nbytes = plan._bind[0]
    rc = int(_native.load().mpc_lqr_step_route(ctypes.byref(p), ctypes.byref(o_), ctypes.byref(out), ws.data_ptr(), nbytes, impl, None))
    if not admitted(impl, pl):
        # 3. refused by code before any launch: the route says so, the call raises, and no output word was written
        assert layout == "pitch_off" and rc == E_DIMS
        with pytest.raises(RuntimeError):
            plan()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(v).all()) if v.dtype != torch.int32 else bool((v == -1).all()) for v in plan.outputs.values())
        return
    # 4. the kernel the case is named for
    assert rc in (AUTO_ROUTE[cid][layout] if impl == 0 else (impl,)), (rc, _native.load().mpc_lqr_last_error())
    resident0 = _native.load().mpc_lqr_resident_launches()
    r = {k: host(v) for k, v in plan().items()}
    if "MPC_DPP16_RESIDENT" in env:
        # the build the case is named for: the resident-F launcher counts its launches (tests/test_gpu_dpp16_resident.py)
        assert _native.load().mpc_lqr_resident_launches() - resident0 == int(env["MPC_DPP16_RESIDENT"] == "1" and "unbounded" in cid)
    # (impl 0: the dense copy may sit on the 16-byte grid where the view does not -- the control runs the kernel the view took, forced)
    ref_plan = run_plan(be, dense, opts_d, impl or rc)
    assert be.step_route(ref_plan)[0] == rc
    ref = {k: host(v) for k, v in ref_plan().items()}
    torch.cuda.synchronize()
    # 1. bitwise the dense call's
    for k in STEP_OUT:
        assert r[k].tobytes() == ref[k].tobytes(), "%s under %s: %s differs from the dense call's" % (cid, layout, k)
    if impl != 0:
        gv = be.lqr_step(*views, opts_v, impl=impl, want_gains=True)
        gd = be.lqr_step(*dense, opts_d, impl=impl, want_gains=True)
        torch.cuda.synchronize()
        for k in ("K", "k", "new_x", "new_u"):
            assert host(gv[k]).tobytes() == host(gd[k]).tobytes(), "%s under %s: %s (gains asked) differs" % (cid, layout, k)
            assert np.isfinite(host(gv[k])).all()
    # 2. the oracle
    o = oracle(d)
    if z is not None and SV.of(layout, "C") not in SHARED and layout != "mixed_b" and layout != "mixed_a":
        check_step(r, o, z)
    hold(r, o, f64)


# ---------------------------------------------------------------------------------------------
# the KKT backward
# ---------------------------------------------------------------------------------------------
def grad_fixture(name, keep_symmetric=False):
    z = golden(name)
    beta = float(z["beta"][0])
    d = {k: z[k] for k in ("C", "c", "F", "x", "u", "dl_dx", "dl_du")}
    d["f"] = z.get("f")
    if keep_symmetric:
        from helpers import asymmetric_problems
        keep = ~asymmetric_problems(z)
        d = {k: (None if v is None else v[:, keep]) for k, v in d.items()}
    d["beta"] = None if np.isnan(beta) else beta
    return d


def grad_random(ns, nc, T, B, seed, beta):
    """A random problem (tests/strided_views.py: random_case) at the solution a few oracle steps reach, rounded to float32."""
    from oracle import lqr_oracle as O
    kw = SV.random_case(ns, nc, T, B, seed)
    pr = {k: SV.f64(kw[k]) for k in ("C", "c", "F", "f", "x_init")}
    x, u = SV.f64(kw["cur_x"]), SV.f64(kw["cur_u"])
    for _ in range(4):
        sol = O.lqr_step(lockstep=False, cur_x=x, cur_u=u, u_lower=None if beta is None else -beta, u_upper=beta, **pr)
        x, u = sol["new_x"], sol["new_u"]
    rng = np.random.default_rng(seed + 1)
    f32 = np.float32
    return dict(C=kw["C"], c=kw["c"], F=kw["F"], f=kw["f"], x=x.astype(f32), u=u.astype(f32),
                dl_dx=rng.standard_normal((T, B, ns)).astype(f32), dl_du=rng.standard_normal((T, B, nc)).astype(f32), beta=beta)


def kkt_route_code(be, blocks, fixed, opts, kernel):
    """mpc_lqr_kkt_fused_kernel_route for exactly what plan_kkt_backward would bind: the kernel's code, or the refusal's."""
    from mpc import _native
    L, _dev, (T, B, ns, nc, n), kw, (x, u, gx, gu), has_f, pf, keep = be._open_kkt(*blocks, *fixed, nominal=False)
    o, keep_o = opts.to_struct(T, B, nc, blocks[0])
    nbytes = int(L.mpc_lqr_kkt_fused_kernel_workspace_bytes(ctypes.byref(pf), ctypes.byref(o), kernel))
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    out = [torch.empty(s, **kw) for s in ((T, B, n, n), (T, B, n), (max(T - 1, 0), B, ns, n), (max(T - 1, 0), B, ns), (B, ns), (T, B, ns), (T, B, nc))]
    ptr = [t.data_ptr() for t in out]
    if not (has_f and T > 1):
        ptr[3] = None
    return int(L.mpc_lqr_kkt_fused_kernel_route(ctypes.byref(pf), ctypes.byref(o), kernel, gx.data_ptr(), gu.data_ptr(), *ptr, None,
                                                ws.data_ptr(), nbytes))


K_DPP16, K_DPP16_PAD, K_MFMA40, K_PAD16, K_PAD4, K_NARROW16, K_NARROW4 = 1, 2, 3, 4, 5, 6, 7
# id -> (builder, fused kernel on the grid (0: the three-call route), fused kernel off it, grads_kernel, layouts)
KKT = {
    "fused-12_4": (lambda: grad_fixture("grad_ns_constrained_f32"), K_DPP16, None, 0, ALL),
    "fused-7_3": (lambda: grad_random(7, 3, 6, 3, 73, 0.4), K_DPP16_PAD, K_DPP16_PAD, 0, ALL),
    "fused-32_8": (lambda: grad_fixture("grad_cfg5_unconstrained_f32"), K_MFMA40, None, 0, ALL),
    "fused-32_8-box": (lambda: grad_fixture("grad_cfg5_constrained_f32"), K_MFMA40, None, 0, ALL),
    "pad-13_4": (lambda: grad_random(13, 4, 6, 3, 134, 0.4), K_PAD4, K_PAD4, 0, ALL),
    "pad-16_4": (lambda: grad_random(16, 4, 6, 3, 164, None), K_PAD16, K_PAD4, 0, ALL),
    "narrow-13_4": (lambda: grad_random(13, 4, 6, 3, 134, 0.4), K_NARROW4, K_NARROW4, 0, ALL),
    "narrow-16_4": (lambda: grad_random(16, 4, 6, 3, 164, None), K_NARROW16, K_NARROW4, 0, ALL),
    "wave-12_4": (lambda: grad_fixture("grad_ns_constrained_f32"), 0, 0, 0, ALL),
    "wave-20_4": (lambda: grad_fixture("grad_asym_20_4_f32", keep_symmetric=True), 0, 0, 0, ALL),
    "generic-f64": (lambda: grad_fixture("grad_constrained_f64"), 0, 0, 0, ALL),
    "generic-nof-f64": (lambda: grad_fixture("grad_constrained_nof_f64"), 0, 0, 0, ALL),
    "wave64-f64": (lambda: grad_fixture("grad_constrained_f64"), 0, 0, 4, ("mixed_a", "mixed_b", "batch_major", "pitch_off")),
}
KKT_PARAMS = [(cid, layout) for cid, case in KKT.items() for layout in case[4]]
_KKT_BUILT = {}


@pytest.mark.parametrize("cid,layout", KKT_PARAMS, ids=["%s-%s" % p for p in KKT_PARAMS])
def test_kkt_backward_on_views(be, cid, layout):
    from mpc._native import StepOptions
    from oracle import lqr_oracle as O
    builder, on_grid, off_grid, grads_kernel, _layouts = KKT[cid]
    if cid not in _KKT_BUILT:
        _KKT_BUILT[cid] = builder()
    g = _KKT_BUILT[cid]
    f64 = g["C"].dtype == np.float64
    T = g["C"].shape[0]
    pl = SV.place_problem(layout, torch, g["C"], g["c"], g["F"] if T > 1 else None, g["f"], device=DEV)
    shows = {r: (None if pl[r] is None else host(pl[r].dense)) for r in "CcFf"}
    beta = g["beta"]
    if beta is not None and not f64:
        beta = float(np.float32(beta))          # the bound as the float32 kernels hold it: a control ON it stays on it for the oracle
    lo, hi = (None, None) if beta is None else (-beta, beta)
    grid = SV.on_grid({r: pl[r] for r in "CcF"}, g["C"].dtype.itemsize)
    kernel = on_grid if grid else off_grid
    fixed = tuple(dev(g[k]) for k in ("x", "u", "dl_dx", "dl_du"))
    view = tuple(None if pl[r] is None else pl[r].view for r in "CcFf")
    dense = tuple(None if pl[r] is None else pl[r].dense for r in "CcFf")
    if not grid:
        # off the 16-byte grid the library routes to other kernels (12/4: kkt_wave for kkt_dpp16, step 8 for 3; 16/4: dword gathers),
        # whose sums run in another order: the dense control goes one element off the grid too, so that both calls run the same kernels
        def nudged(t):
            if t is None:
                return None
            buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
            return buf[1:].view(t.shape).copy_(t)
        dense = tuple(nudged(t) for t in dense)
    opts = StepOptions(u_lower=lo, u_upper=hi, c_symmetric=bool(on_grid))
    if kernel is None:
        # the exact fused kernel off the 16-byte grid: refused by code, nothing launched
        assert kkt_route_code(be, view, fixed, opts, on_grid) == E_DIMS
        assert kkt_route_code(be, tuple(None if pl[r] is None else pl[r].dense for r in "CcFf"), fixed, opts, on_grid) == on_grid
        with pytest.raises(RuntimeError):
            be.plan_kkt_backward(*view, *fixed, opts, kernel=on_grid)
        return
    run = lambda tensors: be.kkt_backward(*tensors, *fixed, opts, kernel=kernel, grads_kernel=grads_kernel)
    a, b = run(view), run(dense)
    torch.cuda.synchronize()
    # (x*, u* are the fixture's: under a layout that shows a broadcast block they are no solution of the shown problem -- the backward
    # is the same linear map of (dl_dx, dl_du) at any point, and the oracle is asked at the same point)
    o = O.kkt_backward(*(SV.f64(shows[r]) for r in "CcFf"), *(SV.f64(g[k]) for k in ("x", "u", "dl_dx", "dl_du")), lo, hi, lockstep=False)
    for k in ("dx_init", "dC", "dc", "dF", "df"):
        if o[k] is None or o[k].size == 0:
            assert a[k] is None or a[k].numel() == 0
            continue
        assert host(a[k]).tobytes() == host(b[k]).tobytes(), "%s under %s: %s differs from the dense call's" % (cid, layout, k)
        scale = max(1.0, np.abs(o[k]).max())
        np.testing.assert_allclose(host(a[k]) / scale, o[k] / scale, rtol=0, atol=1e-10 if f64 else 5e-5, err_msg=k)


# ---------------------------------------------------------------------------------------------
# mpc_traj_cost
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["mixed_a", "mixed_b", "pitch_off"])
@pytest.mark.parametrize("shape", ["12_4-f32", "4_2-f64"])
def test_traj_cost_on_views(be, shape, layout):
    from oracle import lqr_oracle as O
    f64 = shape.endswith("f64")
    if f64:
        z = golden("traj_cost")
        d = dict(C=z["C"], c=z["c"], F=z["F"], f=z["f"], x_init=z["x_init"], cur_u=z["u"])
    else:
        d = SV.random_case(12, 4, 7, 5, 124)
    T = d["C"].shape[0]
    d = dict(d, F=d["F"][:T - 1], f=d["f"][:T - 1])
    pl = SV.place_problem(layout, torch, d["C"], d["c"], d["F"], d["f"], device=DEV)
    x0, u = dev(d["x_init"]), dev(d["cur_u"])
    p, _keep = be._problem(x0, pl["C"].view, pl["c"].view, pl["F"].view, pl["f"].view, None, u)
    assert all(getattr(p, r) == pl[r].view.data_ptr() and getattr(p, r + "_st") == pl[r].st and getattr(p, r + "_sb") == pl[r].sb for r in "CcFf")
    xv, cv = be.traj_cost(x0, u, pl["F"].view, pl["f"].view, pl["C"].view, pl["c"].view)
    xd, cd = be.traj_cost(x0, u, pl["F"].dense, pl["f"].dense, pl["C"].dense, pl["c"].dense)
    torch.cuda.synchronize()
    assert host(xv).tobytes() == host(xd).tobytes() and host(cv).tobytes() == host(cd).tobytes()
    xo, co = O.traj_cost(*(SV.f64(host(t)) for t in (x0, u, pl["F"].dense, pl["f"].dense, pl["C"].dense, pl["c"].dense)))
    # test_traj_cost_parity's tolerances in float64; in float32 test_trajectory_kernels_float32's for x and check_step's for a cost
    np.testing.assert_allclose(host(xv), xo, **(dict(rtol=1e-12, atol=1e-12) if f64 else dict(rtol=2e-4, atol=2e-4)))
    np.testing.assert_allclose(host(cv), co, rtol=1e-12 if f64 else 1e-4)
