"""impl 9 on the device: the NARROW instantiation of the padded 32/8 kernel (one 16-row state tile, n_state <= 16;
csrc/lqr_mfma40_body.h with -DMPC_MFMA40_XT=1).  Against the float64 oracle by the method and numbers of
tests/test_gpu_parity.py::test_padded_mfma40_shapes_between_the_tuned_ones, and against impl 7 on the same call, where every
output is expected bit for bit: the padded kernel's second state tile holds exact zeros at these shapes and the narrow kernel adds
the same numbers in the same order without them."""
import numpy as np
import pytest
import torch

from mpc import _native, mpc, util
from mpc._native import IMPL_MFMA40_NARROW, IMPL_MFMA40_PAD, StepOptions
from mpc.mpc import LinDx, QuadCost

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT = ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alpha_du_norm", "alphas", "qp_iters", "status")


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()
    return _native.HipBackend()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    """bit for bit, +0 and -0 alike (a sum the padded kernel extends by an exact +0 loses the sign of a zero, nothing else)"""
    if a.dtype.is_floating_point:
        return bool(((a.view(torch.int32) == b.view(torch.int32)) | ((a == 0) & (b == 0))).all())
    return bool(torch.equal(a, b))


def case_options(case, p, T, B, nc, g):
    kw = {}
    if case == "bounded":
        kw = dict(u_lower=-0.5, u_upper=0.5)
    elif case == "tensor_bounds":
        kw = dict(u_lower=(-0.5 - torch.rand(T, B, nc, generator=g)).to(DEV), u_upper=(0.5 + torch.rand(T, B, nc, generator=g)).to(DEV))
    elif case == "delta_u":
        kw = dict(u_lower=-0.5, u_upper=0.5, delta_u=0.1)
    elif case == "masked":
        kw = dict(u_zero_I=(torch.rand(T, B, nc, generator=g) < 0.3).to(DEV))
    elif case == "positive_bounds":
        p["cur_u"] = (p["cur_u"].abs() + 0.1).clamp(0.1, 0.6)
        p["cur_x"] = util.get_traj(T, p["cur_u"], p["x_init"], LinDx(p["F"], p["f"])) if T > 1 else p["x_init"][None].clone()
        kw = dict(u_lower=0.1, u_upper=0.6)
    return kw


@pytest.mark.parametrize("case", ["unbounded", "bounded", "tensor_bounds", "delta_u", "masked", "positive_bounds"])
@pytest.mark.parametrize("ns,nc,T,B", [(13, 4, 12, 70), (16, 4, 12, 70), (16, 8, 12, 70), (9, 6, 12, 70), (5, 3, 12, 70),
                                       (16, 4, 1, 70), (16, 4, 12, 1)])
def test_narrow_kernel_against_the_oracle_and_the_padded_kernel(be, ns, nc, T, B, case):
    from oracle import lqr_oracle as O
    import bench
    bounded = case != "unbounded" and case != "masked"
    p = bench.make_problem(ns, nc, T, B, torch.float32, DEV, seed=100 * ns + nc, u_scale=0.3 if bounded else 0.0, clamp=0.4 if bounded else None)
    g = torch.Generator().manual_seed(ns + nc)
    kw = case_options(case, p, T, B, nc, g)
    h = {k: (host(v).astype(np.float64) if v is not None else None) for k, v in p.items()}
    okw = {k: (host(v).astype(np.float64) if torch.is_tensor(v) and v.dtype != torch.bool else (host(v) if torch.is_tensor(v) else v)) for k, v in kw.items()}
    o = O.lqr_step(h["x_init"], h["C"], h["c"], h["F"], h["f"], h["cur_x"], h["cur_u"], okw.get("u_lower"), okw.get("u_upper"),
                   u_zero_I=okw.get("u_zero_I"), delta_u=okw.get("delta_u"), lockstep=False, return_gains=True, nthreads=O.max_threads())
    args = (p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"])
    assert be.impl_supported(ns, nc, torch.float32, IMPL_MFMA40_NARROW)
    for vouch in (False, True):
        opts = StepOptions(nominal_on_dynamics=vouch, c_symmetric=vouch, **kw)
        r9 = be.lqr_step(*args, opts, impl=IMPL_MFMA40_NARROW, want_gains=not vouch)
        r7 = be.lqr_step(*args, opts, impl=IMPL_MFMA40_PAD, want_gains=not vouch)
        torch.cuda.synchronize()
        same = np.isclose(host(r9["alphas"]), o["alphas"], rtol=1e-5)
        assert (~same).sum() <= 1
        for k in ("new_x", "new_u"):
            np.testing.assert_allclose(host(r9[k])[:, same], o[k][:, same], rtol=1e-3, atol=1e-4, err_msg="%s %s" % (k, "vouched" if vouch else "bare"))
        np.testing.assert_allclose(host(r9["costs"])[same], o["costs"][same], rtol=2e-4)
        np.testing.assert_allclose(host(r9["old_costs"]), o["old_costs"], rtol=1e-5)
        np.testing.assert_allclose(host(r9["full_du_norm"]), o["full_du_norm"], rtol=1e-3, atol=1e-4)
        assert (host(r9["status"]) & 3 == 0).all()
        if not vouch:
            np.testing.assert_allclose(host(r9["K"]), o["K"], rtol=1e-3, atol=1e-4)
            np.testing.assert_allclose(host(r9["k"]), o["k"], rtol=1e-3, atol=1e-4)
        # ... and the padded kernel on the same call: every output, bit for bit
        for k in OUT + (("K", "k") if not vouch else ()):
            assert same_bits(r9[k], r7[k]), (k, vouch, (r9[k].double() - r7[k].double()).abs().max().item())


def test_forced_narrow_kernel_reports_a_nonsymmetric_C_as_the_padded_one(be):
    import bench
    ns, nc, T, B = 13, 4, 8, 5
    p = bench.make_problem(ns, nc, T, B, torch.float32, DEV, seed=5)
    p["C"][3, 2, 1, ns + 1] += 0.5
    args = (p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"])
    r9 = be.lqr_step(*args, StepOptions(), impl=IMPL_MFMA40_NARROW)
    r7 = be.lqr_step(*args, StepOptions(), impl=IMPL_MFMA40_PAD)
    torch.cuda.synchronize()
    assert ((host(r9["status"]) & _native.ST_C_ASYMMETRIC) != 0).tolist() == [False, False, True, False, False]
    assert torch.equal(r9["status"], r7["status"])


def test_step_started_from_the_qp_record_gives_the_cold_steps_result(be):
    import bench
    ns, nc, T, B = 16, 4, 12, 70
    p = bench.make_problem(ns, nc, T, B, torch.float32, DEV, seed=9, u_scale=0.3, clamp=0.4)
    args = (p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"])
    kw = dict(u_lower=-0.5, u_upper=0.5, nominal_on_dynamics=True, c_symmetric=True)
    plan = be.plan_step(*args, StepOptions(**kw), impl=IMPL_MFMA40_NARROW)
    assert be.step_route(plan)[0] == IMPL_MFMA40_NARROW
    cold = {k: v.clone() for k, v in plan().items() if torch.is_tensor(v)}
    rec = be.qp_record(plan)
    assert rec is not None and tuple(rec.shape) == (T, B, nc)
    p7 = be.plan_step(*args, StepOptions(**kw), impl=IMPL_MFMA40_PAD)
    rec7 = be.qp_record(p7)
    assert rec.stride() == rec7.stride() and rec.storage_offset() == rec7.storage_offset()
    warm_plan = be.plan_variant(plan, opts=StepOptions(qp_start=rec, **kw))
    warm = warm_plan()
    torch.cuda.synchronize()
    assert torch.equal(warm["alphas"], cold["alphas"])
    np.testing.assert_allclose(host(warm["new_u"]), host(cold["new_u"]), rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(host(warm["new_x"]), host(cold["new_x"]), rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(host(warm["costs"]), host(cold["costs"]), rtol=2e-4)
    # a warm start costs no more trips of the QP than the cold one
    assert int(warm["qp_iters"].sum()) <= int(cold["qp_iters"].sum())


@pytest.mark.parametrize("bounded", [False, True], ids=["unbounded", "bounded"])
def test_sweep_only_writes_the_gains_and_no_trajectory(be, bounded):
    import bench
    ns, nc, T, B = 13, 4, 12, 70
    p = bench.make_problem(ns, nc, T, B, torch.float32, DEV, seed=3, u_scale=0.3 if bounded else 0.0, clamp=0.4 if bounded else None)
    args = (p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"])
    kw = dict(u_lower=-0.5, u_upper=0.5) if bounded else {}
    full = be.lqr_step(*args, StepOptions(**kw), impl=IMPL_MFMA40_NARROW, want_gains=True)
    so = StepOptions(**kw)
    so.sweep_only = True
    ox, ou = torch.full((T, B, ns), 7.0, device=DEV), torch.full((T, B, nc), 7.0, device=DEV)
    sw = be.lqr_step(*args, so, impl=IMPL_MFMA40_NARROW, want_gains=True, out_x=ox, out_u=ou)
    torch.cuda.synchronize()
    assert torch.equal(sw["K"], full["K"]) and torch.equal(sw["k"], full["k"])
    assert torch.equal(sw["old_costs"], full["old_costs"]) and torch.equal(sw["qp_iters"], full["qp_iters"])
    assert bool((ox == 7.0).all()) and bool((ou == 7.0).all())


def _solve(kind, flag, monkeypatch, shared_cost=False, asym=False):
    plans = []
    orig = _native.HipBackend.plan_step

    def spy(self, *a, **k):
        plan = orig(self, *a, **k)
        plans.append(plan)
        return plan
    monkeypatch.setattr(_native.HipBackend, "plan_step", spy)
    g = torch.Generator().manual_seed(41)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    if kind == "slew":                   # the 12/4 -> 16/4 case of tests/test_gpu_slew_planned.py
        ns, nc, T, B = 12, 4, 6, 9
    else:
        ns, nc, T, B = 13, 4, 6, 9
    n = ns + nc
    L = r(n, n) if shared_cost else r(T, B, n, n)
    C = (L @ L.transpose(-1, -2) + torch.eye(n, dtype=torch.float64)).float().to(DEV)
    if asym:                             # one C_t of one problem is not symmetric
        C[2, 4, 1, n - 1] += 0.5
    c = (r(n) if shared_cost else r(T, B, n)).float().to(DEV)
    F = (0.2 * r(T - 1, B, ns, n) + torch.cat((torch.eye(ns, dtype=torch.float64), torch.zeros(ns, nc, dtype=torch.float64)), 1)).float().to(DEV)
    f = (0.1 * r(T - 1, B, ns)).float().to(DEV)
    x0 = r(B, ns).float().to(DEV)
    prev = (0.2 * r(B, nc)).float().to(DEV)
    extra = dict(slew_rate_penalty=1.0, prev_ctrl=prev) if kind == "slew" else {}
    ctrl = mpc.MPC(ns, nc, T, u_lower=-0.3, u_upper=0.3, lqr_iter=5, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                   n_batch=B, narrow_step_kernel=flag, **extra)
    with torch.no_grad():
        x, u, costs = ctrl(x0, QuadCost(C, c), LinDx(F, f))
    torch.cuda.synchronize()
    monkeypatch.setattr(_native.HipBackend, "plan_step", orig)
    return x, u, costs, [_native.HipBackend.step_route(pl)[0] for pl in plans]


@pytest.mark.parametrize("kind,shared_cost", [("slew", False), ("slew", True), ("lin", False)])
def test_whole_solves_with_the_flag_run_impl_9_and_equal_the_flag_off_solve(be, monkeypatch, kind, shared_cost):
    x9, u9, c9, routes9 = _solve(kind, True, monkeypatch, shared_cost)
    x0, u0, c0, routes0 = _solve(kind, False, monkeypatch, shared_cost)
    assert routes9 and all(k == IMPL_MFMA40_NARROW for k in routes9), routes9
    assert routes0 and all(k == IMPL_MFMA40_PAD for k in routes0), routes0
    assert int((u9.abs() == 0.3).sum()) > 0
    assert same_bits(x9, x0) and same_bits(u9, u0) and same_bits(c9, c0)


@pytest.mark.parametrize("kind", ["slew", "lin"])
def test_a_nonsymmetric_C_gives_the_flag_off_solve(be, monkeypatch, kind):
    """A forced kernel only flags a C_t that is not symmetric, impl 0 solves that problem again on the generic kernel: the
    narrow-bound loop starts over on auto plans when its first step reports the bit, and x, u and costs are the flag-off solve's."""
    x9, u9, c9, routes9 = _solve(kind, True, monkeypatch, asym=True)
    x0, u0, c0, routes0 = _solve(kind, False, monkeypatch, asym=True)
    assert routes9 == [IMPL_MFMA40_NARROW, IMPL_MFMA40_PAD], routes9           # bound to 9, then again under impl 0
    assert routes0 == [IMPL_MFMA40_PAD], routes0
    assert torch.equal(x9, x0) and torch.equal(u9, u0) and torch.equal(c9, c0)
    # (the problem was worth the trouble: read through its symmetry, that C gives another answer)
    xs, us, _, _ = _solve(kind, False, monkeypatch, asym=False)
    assert not torch.equal(us[:, 4], u0[:, 4])


@pytest.mark.parametrize("asym", [False, True], ids=["symmetric", "nonsymmetric"])
def test_network_slew_loop_with_the_flag_sweeps_on_impl_9_and_equals_the_flag_off_solve(be, monkeypatch, asym):
    """`planned_network_slew`: NNDynamics(12, 4) with a penalty runs `_iterate_network` at 16/4; with `narrow_step_kernel` its
    sweep (MPC_OPT_SWEEP_ONLY) is bound to impl 9 -- and bound again under impl 0 where C is not symmetric."""
    from mpc.dynamics import NNDynamics
    ns, nc, T, B, n = 12, 4, 6, 9, 16
    torch.manual_seed(3)
    dyn = NNDynamics(ns, nc, [32], activation="sigmoid").to(DEV)
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    L = r(T, B, n, n)
    C = (L @ L.transpose(2, 3) / n + torch.eye(n)).to(DEV)
    if asym:
        C[2, 4, 1, n - 1] += 0.5
    c, x0 = r(T, B, n).to(DEV), r(B, ns).to(DEV)
    impls = []
    orig = _native.HipBackend.plan_network_iteration

    def spy(self, *a, **k):
        impls.append(k.get("impl", 0))
        return orig(self, *a, **k)
    monkeypatch.setattr(_native.HipBackend, "plan_network_iteration", spy)
    outs = []
    for flag in (True, False):
        ctrl = mpc.MPC(ns, nc, T, u_lower=-0.3, u_upper=0.3, lqr_iter=5, verbose=-1, exit_unconverged=False, detach_unconverged=False,
                       backprop=False, slew_rate_penalty=1.0, eps=0.0, grad_method=mpc.GradMethods.ANALYTIC, planned_network_slew=True,
                       narrow_step_kernel=flag)
        with torch.no_grad():
            outs.append(ctrl(x0, QuadCost(C, c), dyn))
    torch.cuda.synchronize()
    assert impls == ([IMPL_MFMA40_NARROW, 0, 0] if asym else [IMPL_MFMA40_NARROW, 0]), impls
    for a, b in zip(*outs):
        assert torch.equal(a, b)
