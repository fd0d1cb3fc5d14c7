"""Every kernel that parks data in a global workspace and fetches it back through its staging ring, launched MANY times on one plan.

docs/history/r22.md found MPC_KKT_MFMA40_NARROW16 returning one to three whole problems wrong in about 0.4 % of its launches while the
suite, which launches every kernel once per case, passed 1755 of 1755.  A fault of that kind is a race against the memory system:
it shows in a fraction of the launches, on another problem each time.  So each case here

  1. binds one plan, launches it once and holds that launch to the float64 oracle (the helpers and numbers of
     tests/test_gpu_narrow_kkt.py for the fused backwards, tests/test_gpu_fullsize.py::strict_step_check for the steps) and, for the
     one-state-tile kernels, to the two-tile kernel on the same tensors, bit for bit;
  2. launches R more times with nothing changed and compares every output (the fused 32/8 family: every part of the plan's workspace
     too) with the first launch's clone ON THE DEVICE, as int32 so that a NaN cannot hide a difference, adding into small device
     tensors of mismatch counts; the host synchronises once and reads them once, after the last launch;
  3. passes when every count is zero.

Batches.  One problem runs per wavefront (four per wavefront in the 12/4 kernels) and the arithmetic does not depend on the problem's
index, so a batch that repeats the 12 vouched problems k times must give, copy for copy, the bits of the B = 12 launch: asserted once,
directly, and the repeats of that batch are then held to those vouched bits.  The repeats run at B = 12 (where r22 saw the miss) and at
a B that puts more wavefronts on the chip than it holds at once (256 CUs): 4104 for the one-tile kernels (12 wavefronts a CU by their
13.3 KiB of LDS: 3072), 2064 for the two-tile ones (at most 6 a CU by their 26.6 - 31.5 KiB: 1536), 9216 for the 12/4 kernels (at most
8 wavefronts of 4 problems a CU: 8192), 4092 for the resident-F build (routed up to one wavefront per SIMD: 4096 problems).

Cold caches.  Every launch runs behind a 512 MiB write (twice the last-level cache).  Launched back to back on warm caches the parent's
NARROW16 did not miss once in 26,000 launches at B = 12 -- r22's repeats rebuilt their tensors every time --; behind the write it does.

R, from misses per launch measured on the library BEFORE the fix (one MI355X, docs/history/r24.md has the whole table):
  tiled, cold    NARROW16 1000 of 1000 launches (9.9 problems a launch), impl 9 with a box 738 of 1000, impl 9 without 611 of 1000.
                 R_TILED = 100 passes the least of them with probability 0.389^100 < 1e-40, and any kernel that misses in one launch of
                 15 with (14/15)^100 = 1.0e-3; 0.1 - 0.5 s a case.  (Warm: 1000, 119 and 29 of 1000.)
  B = 12, cold   NARROW16 4 of 6000 (6.7e-4 a launch), NARROW4 2 of 4000, impl 9 3 and 5 of 6000.  Passing with probability 1e-3 takes
                 R = 10,300 at that rate, 8 s a case: the batch was raised instead (above), and R_SMALL = 3000 (2.3 s) is what a few
                 seconds buy here: it catches the parent's NARROW16 with probability 1 - (1 - 6.7e-4)^3000 = 0.87.
  NARROW4        missed ONLY at small batches (2 of 4000 at B = 12 cold, 1 of 1000 at B = 384; none in 1000 at 1536 and 4104, warm or
                 cold): its B = 12 case catches the parent's with probability 1 - (1 - 5e-4)^3000 = 0.78, no batch measured does better
                 within seconds.  Same defect, same source line as the two above, which are caught with certainty.
  Every other kernel of the table: no miss in 4000 launches at B = 12 and 200 at its tiled batch (warm), before or after.

The failure message names the launches, problems and outputs that differ and, for the 32/8 family, which parts of the workspace
(K | k | V | v,g | dx | du at T B kf40_off(xt, part) floats, csrc/lqr_params.h) differ from the first launch's: parts that differ mean a
wrong sweep, equal parts under differing outputs a wrong read-back."""
import time

import numpy as np
import pytest
import torch

from mpc import _native
from mpc._native import (IMPL_DPP16, IMPL_DPP16_PAD, IMPL_MFMA40_NARROW, IMPL_MFMA40_PAD, KKT_DPP16, KKT_DPP16_PAD, KKT_MFMA40,
                         KKT_MFMA40_NARROW4, KKT_MFMA40_NARROW16, KKT_MFMA40_PAD4, KKT_MFMA40_PAD16, KKT_NONE, StepOptions)
from test_gpu_narrow_kkt import GRADS, check_oracle, on_device, plan_for, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_OUT = ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alpha_du_norm", "alphas", "qp_iters", "status")
B0 = 12
TILED = {"narrow": 4104, "wide": 2064, "dpp16": 9216, "resident": 4092}
# launches after the first, by batch: see the module docstring and docs/history/r24.md
R_SMALL, R_TILED = 3000, 100


# the fused 32/8 backward's workspace on xt state tiles, floats a problem-step (csrc/lqr_params.h, kf40_words / kf40_off)
def kf40_parts(xt):
    return (("K", 8 * 16 * xt), ("k", 8), ("V", 256 * xt * xt), ("v,g", 32 * xt), ("dx", 16 * xt), ("du", 8))


assert sum(w for _, w in kf40_parts(1)) == 448 and sum(w for _, w in kf40_parts(2)) == 1392


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()
    return _native.HipBackend()


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def _kkt(name, ns, nc, T, ask, want, family, xt=0, twin=None):
    return pytest.param(dict(kind="kkt", ns=ns, nc=nc, T=T, ask=ask, want=want, family=family, xt=xt, twin=twin), id=name)


def _step(name, ns, nc, T, impl, family, bounded, twin=None, resident=False):
    return pytest.param(dict(kind="step", ns=ns, nc=nc, T=T, impl=impl, family=family, bounded=bounded, twin=twin, resident=resident), id=name)


CASES = [
    _kkt("kkt-narrow16", 16, 4, 70, KKT_MFMA40_NARROW16, KKT_MFMA40_NARROW16, "narrow", xt=1, twin=KKT_MFMA40_PAD16),
    _kkt("kkt-narrow4", 13, 4, 70, KKT_MFMA40_NARROW4, KKT_MFMA40_NARROW4, "narrow", xt=1, twin=KKT_MFMA40_PAD4),
    _kkt("kkt-pad16", 16, 4, 70, KKT_MFMA40_PAD16, KKT_MFMA40_PAD16, "wide", xt=2),
    _kkt("kkt-pad4", 13, 4, 70, KKT_MFMA40_PAD4, KKT_MFMA40_PAD4, "wide", xt=2),
    _kkt("kkt-exact-32-8", 32, 8, 70, KKT_NONE, KKT_MFMA40, "wide", xt=2),
    # the 12/4 kernels keep their gains in registers up to 64 timesteps and in the record beyond: both horizons
    _kkt("kkt-12-4-T70", 12, 4, 70, KKT_NONE, KKT_DPP16, "dpp16"),
    _kkt("kkt-12-4-T50", 12, 4, 50, KKT_NONE, KKT_DPP16, "dpp16"),
    _kkt("kkt-8-4-T70", 8, 4, 70, KKT_NONE, KKT_DPP16_PAD, "dpp16"),
    _kkt("kkt-8-4-T50", 8, 4, 50, KKT_NONE, KKT_DPP16_PAD, "dpp16"),
    # steps, vouched (c_symmetric, nominal_on_dynamics): the rollout reads K, k back.  Scalar bounds (the priced rollout) and none (the lean one)
    _step("step-impl7-box", 13, 4, 70, IMPL_MFMA40_PAD, "wide", True),
    _step("step-impl7-free", 13, 4, 70, IMPL_MFMA40_PAD, "wide", False),
    _step("step-impl9-box", 16, 4, 70, IMPL_MFMA40_NARROW, "narrow", True, twin=IMPL_MFMA40_PAD),
    _step("step-impl9-free", 16, 4, 70, IMPL_MFMA40_NARROW, "narrow", False, twin=IMPL_MFMA40_PAD),
    _step("step-impl8-box-T70", 10, 3, 70, IMPL_DPP16_PAD, "dpp16", True),
    _step("step-impl8-free-T70", 10, 3, 70, IMPL_DPP16_PAD, "dpp16", False),
    _step("step-impl8-box-T50", 10, 3, 50, IMPL_DPP16_PAD, "dpp16", True),
    _step("step-impl8-free-T50", 10, 3, 50, IMPL_DPP16_PAD, "dpp16", False),
    _step("step-12-4-box-T70", 12, 4, 70, IMPL_DPP16, "dpp16", True),
    _step("step-12-4-free-T70", 12, 4, 70, IMPL_DPP16, "dpp16", False),
    _step("step-12-4-box-T50", 12, 4, 50, IMPL_DPP16, "dpp16", True),
    _step("step-12-4-free-T50", 12, 4, 50, IMPL_DPP16, "dpp16", False),
    _step("step-12-4-resident-F", 12, 4, 50, IMPL_DPP16, "resident", False, resident=True),
]


# ---------------------------------------------------------------------------------------------
# comparing on the device
# ---------------------------------------------------------------------------------------------
def by_problem(t, axis):
    """[before, B, after] int32 (float32 by its bits) view of a contiguous tensor whose batch axis is `axis`"""
    assert t.is_contiguous()
    v = t.view(torch.int32) if t.dtype == torch.float32 else t
    assert v.dtype == torch.int32, v.dtype
    before = int(np.prod(t.shape[:axis], dtype=np.int64))
    return v.reshape(before, t.shape[axis], -1)


def workspace_parts(ws, T, B, xt):
    """the parts of a fused 32/8 backward's workspace as [T, B, words] views"""
    w32 = ws[:ws.numel() // 4 * 4].view(torch.float32)
    views, at = [], 0
    for name, words in kf40_parts(xt):
        assert (at + words) * T * B <= w32.numel(), "the workspace is smaller than csrc/lqr_params.h says"
        views.append(("workspace " + name, by_problem(w32[at * T * B:(at + words) * T * B].view(T, B, words), 1)))
        at += words
    return views


def repeat_on_device(launch, views, first, R, flush=None):
    """`launch()` R times; after each, every view against `first` (the bits the caller has vouched for).  flush: a large tensor that is
    overwritten in front of every launch, so that the launch finds none of its data in the caches.
    -> (counts [n_views, B], elements [R, n_views], problems [R]) on the host, after one synchronisation."""
    B = views[0][1].shape[1]
    counts = torch.zeros(len(views), B, dtype=torch.int32, device=DEV)
    elements = torch.zeros(R, len(views), dtype=torch.int32, device=DEV)
    problems = torch.zeros(R, dtype=torch.int32, device=DEV)
    total = torch.zeros(B, dtype=torch.int32, device=DEV)
    for r in range(R):
        if flush is not None:
            flush.add_(1)
        launch()
        total.zero_()
        for i, (_, v) in enumerate(views):
            s = (v != first[i]).sum(dim=(0, 2), dtype=torch.int32)
            counts[i] += s
            total += s
            elements[r, i] = s.sum()
        problems[r] = (total > 0).sum()
    torch.cuda.synchronize()
    return counts.cpu().numpy(), elements.cpu().numpy(), problems.cpu().numpy()


def describe(names, counts, elements, problems, n_out):
    """what differed from the first launch: launches, problems, outputs; workspace parts (views n_out ..) apart"""
    R = len(problems)
    missed = np.nonzero(problems)[0]
    if missed.size == 0:
        return "%d launches, all equal to the first" % R
    lines = ["%d of %d launches differ from the first (%.2e a launch; %.2f problems in each on average): launches %s%s"
             % (missed.size, R, missed.size / R, problems[missed].mean(), missed[:20].tolist(), " ..." if missed.size > 20 else "")]
    for r in missed[:5]:
        lines.append("  launch %d: %d problems; elements by output %s" % (r, problems[r], {names[i]: int(elements[r, i]) for i in np.nonzero(elements[r])[0]}))
    for i, name in enumerate(names):
        bad = np.nonzero(counts[i])[0]
        if bad.size:
            lines.append("  %s: %d problems differed at some launch: %s%s" % (name, bad.size, bad[:24].tolist(), " ..." if bad.size > 24 else ""))
    if len(names) > n_out:
        differ = [names[i] for i in range(n_out, len(names)) if counts[i].any()]
        equal = [names[i] for i in range(n_out, len(names)) if not counts[i].any()]
        lines.append("  workspace parts that differ: %s; equal: %s" % (differ or "none", equal or "none"))
        out_only = sum(1 for r in missed if elements[r, :n_out].any() and not elements[r, n_out:].any())
        lines.append("  => %d of the launches that missed left the whole workspace as the first launch did (a wrong read-back); the others "
                     "parked other numbers (a wrong sweep)" % out_only)
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------
# one case: bind, vouch for the first launch, hand back what to repeat
# ---------------------------------------------------------------------------------------------
def tile(t, k):
    """a [T, B0, ...] tensor with its batch repeated k times: problem j * B0 + i is problem i"""
    return t if t is None or k == 1 else t.repeat(1, k, *([1] * (t.dim() - 2))).contiguous()


def copies_differ(big, small, k):
    """'' where every copy of the tiled batch holds the bits of the B = 12 launch, else which (copy, problem) do not"""
    lines = []
    for (name, a), (_, b) in zip(big, small):
        x, y = a.reshape(a.shape[0], k, B0, -1), b.reshape(b.shape[0], 1, B0, -1)
        if not bool((x == y).all()):
            bad = torch.nonzero((x != y).any(dim=3).any(dim=0))
            lines.append("%s: the first launch of the tiled batch differs from the B = 12 launch at (copy, problem) %s%s"
                         % (name, bad[:12].tolist(), " ..." if bad.shape[0] > 12 else ""))
    return "\n".join(lines)


def tiled_reference(small, k):
    """the B = 12 launch's bits, copy for copy, in the tiled batch's order"""
    return [b.repeat(1, k, 1) for _, b in small]


def kkt_views(plan, T, B, xt):
    g = plan.outputs
    views = [(k, by_problem(g[k], 0 if k == "dx_init" else 1)) for k in GRADS if g[k] is not None and g[k].numel()]
    n_out = len(views)
    if xt:
        views += workspace_parts(g["_keep"][2], T, B, xt)
    return views, n_out


def bind_kkt(be, case, k):
    ns, nc, T = case["ns"], case["nc"], case["T"]
    z = reference(ns, nc, T, B0, "scalar", True)
    d0 = on_device(z)
    d = {key: (tile(v, k) if torch.is_tensor(v) else v) for key, v in d0.items()}
    kw = dict(kernel=case["ask"]) if case["ask"] != KKT_NONE else {}
    small = plan_for(be, d0, **kw)
    assert small.kernel == case["want"] == be.kkt_route(small), (small.kernel, case["want"])
    got = small()
    torch.cuda.synchronize()
    check_oracle(got, z["oracle"], "first launch at B = 12")
    if case["twin"] is not None:                       # the two-tile kernel on the same tensors: equality, as tests/test_gpu_narrow_kkt.py demands
        wide = plan_for(be, d0, kernel=case["twin"])
        assert wide.kernel == case["twin"]
        ref = wide()
        torch.cuda.synchronize()
        for key in GRADS:
            if ref[key] is not None and ref[key].numel():
                assert torch.equal(got[key], ref[key]), "%s differs from the two-tile kernel's" % key
    if k == 1:
        plan = small
    else:
        plan = plan_for(be, d, **kw)
        assert plan.kernel == case["want"] == be.kkt_route(plan)
        plan()
        torch.cuda.synchronize()
    views, n_out = kkt_views(plan, T, k * B0, case["xt"])
    return plan, views, n_out, kkt_views(small, T, B0, 0)[0], (d0, d, small)


def step_views(plan):
    o = plan.outputs
    return [(key, by_problem(o[key], 1 if o[key].dim() == 3 else 0)) for key in STEP_OUT]


def bind_step(be, case, k, monkeypatch):
    import bench
    from oracle import lqr_oracle as O
    from test_gpu_fullsize import h64, strict_step_check
    ns, nc, T, impl, bounded = case["ns"], case["nc"], case["T"], case["impl"], case["bounded"]
    dpp = case["family"] in ("dpp16", "resident")
    # the problems of tests/test_gpu_fullsize.py (12/4 family: bounds +-1) and of tests/test_gpu_narrow.py (32/8 family: +-0.5)
    clamp, bound = (1.0, 1.0) if dpp else (0.4, 0.5)
    p0 = bench.make_problem(ns, nc, T, B0, torch.float32, DEV, seed=100 * ns + nc, u_scale=0.3 if bounded else 0.0, clamp=clamp if bounded else None)
    kw = dict(u_lower=-bound, u_upper=bound) if bounded else {}
    opts = StepOptions(nominal_on_dynamics=True, c_symmetric=True, **kw)
    h = {key: h64(v) for key, v in p0.items()}
    # (the fused float32 12/4 kernels start every box QP cold: the oracle with the same start, as tests/test_gpu_fullsize.py holds them)
    o = O.lqr_step(h["x_init"], h["C"], h["c"], h["F"], h["f"], h["cur_x"], h["cur_u"], lockstep=False, nthreads=O.max_threads(),
                   return_gains=True, qp_cold=bounded and dpp, **kw)
    if case["resident"]:
        monkeypatch.setenv("MPC_DPP16_RESIDENT", "1")
    args = lambda p: (p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"])

    def bound_plan(p, which):
        plan = be.plan_step(*args(p), opts, impl=which)
        assert be.step_route(plan)[0] == which, (be.step_route(plan), which)
        for key in STEP_OUT:
            plan.outputs[key].fill_(float("nan") if plan.outputs[key].dtype.is_floating_point else -1)
        return plan
    small = bound_plan(p0, impl)
    n0 = _native.load().mpc_lqr_resident_launches()
    r = small()
    torch.cuda.synchronize()
    if case["resident"]:
        assert _native.load().mpc_lqr_resident_launches() == n0 + 1, "the launch did not take the resident-F build"
    # (beyond 65 timesteps: the tolerance tests/test_gpu_fullsize.py states for these kernels there)
    tol = dict(rtol=2e-3, atol=5e-4) if T > 65 else {}
    strict_step_check("repeat_%s" % case["family"], r, o, B0, have_gains=False, cost_atol=3e-7 * float(np.abs(o["old_costs"]).max()), **tol)
    np.testing.assert_allclose(r["old_costs"].cpu().numpy(), o["old_costs"], rtol=2e-5)
    if case["twin"] is not None:                       # impl 7 on the same call, bit for bit (+0 and -0 alike): tests/test_gpu_narrow.py
        from test_gpu_narrow import same_bits
        ref = bound_plan(p0, case["twin"])()
        torch.cuda.synchronize()
        for key in STEP_OUT:
            assert same_bits(r[key], ref[key]), "%s differs from the two-tile kernel's" % key
    if k == 1:
        return small, step_views(small), len(STEP_OUT), step_views(small), (p0, small)
    p = {key: (tile(v, k) if v.dim() > 2 else v.repeat(k, 1).contiguous()) for key, v in p0.items()}
    plan = bound_plan(p, impl)
    n0 = _native.load().mpc_lqr_resident_launches()
    plan()
    torch.cuda.synchronize()
    if case["resident"]:
        assert _native.load().mpc_lqr_resident_launches() == n0 + 1, "the tiled launch did not take the resident-F build"
    return plan, step_views(plan), len(STEP_OUT), step_views(small), (p0, p, small)


FLUSH_BYTES = 512 << 20          # twice the 256 MiB of the last-level cache


def run_case(be, case, tiled, R, monkeypatch=None, cold=True):
    """One case: bind (the binder launches once and vouches for that launch), then R more launches.  cold: every launch behind a
    write of FLUSH_BYTES, so that it finds nothing of its problem in the caches.
    -> (report, counts, problems per launch, seconds spent in the R launches); the soak of docs/history/r24.md calls this with its own R"""
    k = TILED[case["family"]] // B0 if tiled else 1
    assert k * B0 == (TILED[case["family"]] if tiled else B0)
    if case["kind"] == "kkt":
        plan, views, n_out, small, keep = bind_kkt(be, case, k)
    else:
        plan, views, n_out, small, keep = bind_step(be, case, k, monkeypatch)
    first = [v.clone() for _, v in views]
    note = ""
    if k > 1:
        # the tiled batch against the B = 12 launch, once and directly; the repeats are then held to those vouched bits (the workspace,
        # which only serves to tell a wrong sweep from a wrong read-back, to the first tiled launch's)
        note = copies_differ(views[:n_out], small, k)
        first[:n_out] = tiled_reference(small, k)
    flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device=DEV) if cold else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counts, elements, problems = repeat_on_device(plan, views, first, R, flush)
    dt = time.perf_counter() - t0
    names = [n for n, _ in views]
    print("B = %d, R = %d%s: %.2f s; %d launches with a miss, %d problem-launches"
          % (k * B0, R, ", cold caches" if cold else "", dt, int((problems > 0).sum()), int(problems.sum())))
    report = describe(names, counts, elements, problems, n_out)
    return (note + "\n" if note else "") + report, counts, problems, dt, note


@pytest.mark.parametrize("batch", ["B12", "tiled"])
@pytest.mark.parametrize("case", CASES)
def test_every_launch_on_one_plan_gives_the_bits_of_the_first(be, case, batch, monkeypatch):
    tiled = batch == "tiled"
    report, counts, problems, _, note = run_case(be, case, tiled, R_TILED if tiled else R_SMALL, monkeypatch)
    print(report)
    ok = not note and not bool(counts.any()) and not bool(problems.any())
    assert ok, report
