"""CPU: the kernel SOURCES on strided C, c, F, f (and qp_start) views, through the wavefront emulator (tests/emu_backend.py,
tests/emu_narrow.py with layouts=...).  tests/strided_views.py carves every tensor out of its own NaN-filled arena, each through its
own (st, sb) pair, so a site that takes c_st for f_st, C_sb for F_sb, assumes st = B sb or st >= sb, or reads a neighbour's block
shows here as a differing bit or a NaN -- in a test process, before a device sees the kernel.

Per emulated kernel and per layout its support rule (csrc/lqr_rules.hip) admits:
  (a) every output is BITWISE the same emulated kernel's on the dense copy of the same values (layouts=None: the drivers as ever);
  (b) the oracle comparison of that kernel's own emulator test (tests/test_emu_mfma16.py, tests/test_emu_narrow.py), at its tolerances.
A shared layout shows the broadcast block's values: the case (nominal, oracle) is then built from those.
Every layout on one fixture per kernel, the two mixed ones on a second; T just above the kernel's ring depth."""
import numpy as np
import pytest

import strided_views as SV
from conftest import golden

STEP_OUT = ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alpha_du_norm", "alphas", "qp_iters", "status", "K", "k")


@pytest.fixture(scope="module")
def emu(emu_libs):
    import emu_backend
    emu_backend.lib()
    return emu_backend


f64, cut, renominal, random_case, shown = SV.f64, SV.cut, SV.renominal, SV.random_case, SV.shown


def bitwise(a, b, keys, what):
    for k in keys:
        if a.get(k) is None:
            assert b.get(k) is None
            continue
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs from the dense call's, first at %s" % (
            what, k, np.argwhere(~((a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))))[:3].tolist())


def oracle_step(d):
    from oracle import lqr_oracle as O
    return O.lqr_step(lockstep=False, return_gains=True, **{k: (f64(v) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in d.items()})


def hold_step(r, o, d):
    """The oracle comparison of test_emulated_kernel_matches_oracle_and_reference / test_emulated_dpp16_matches_oracle_and_reference."""
    assert (r["status"] & 2 == 0).all()
    assert (r["status"] & 4 == 0).all()      # the nominal IS the rollout of its controls through the F, f the view shows
    f32 = d["C"].dtype == np.float32
    atol = 1e-3 if (d.get("u_lower") is not None and f32) else 1e-4
    for k in ("K", "k", "new_x", "new_u"):
        np.testing.assert_allclose(r[k], o[k], rtol=1e-3, atol=atol, err_msg=k)
    np.testing.assert_allclose(r["costs"], o["costs"], rtol=1e-4)
    np.testing.assert_allclose(r["old_costs"], o["old_costs"], rtol=1e-4)
    np.testing.assert_allclose(r["alphas"], o["alphas"], rtol=1e-6)
    np.testing.assert_allclose(r["full_du_norm"], o["full_du_norm"], rtol=2e-3, atol=2e-4)


def admitted(kernel, layout, kw):
    """csrc/lqr_rules.hip: the exact 12/4 and 32/8 kernels and the 16-byte gathers stream 16-byte granules -- the first block and
    both strides of C, c, F, f on 16 bytes (the gathers: of C and F, and sizes in fours); every other kernel takes any layout."""
    if kernel in ("dpp16", "dpp16_ring2", "mfma40", "mfma40_ring2"):
        roles = ("C", "c", "F", "f")
    elif kernel in ("mfma40_pad16", "narrow16"):
        roles = ("C", "F")
    else:
        return True
    pl = SV.place_problem(layout, np, kw["C"], kw["c"], kw["F"], kw.get("f"))
    return SV.on_grid({r: pl[r] for r in roles}, 4)


def run_step(emu, kernel, d, layouts, qp_start=None, dtype=np.float32):
    if kernel in ("narrow4", "narrow16"):
        import emu_narrow
        assert qp_start is None
        return emu_narrow.step(emu_narrow.lib(int(kernel[6:])), d["x_init"], d["C"], d["c"], d["F"], d.get("f"), d["cur_x"], d["cur_u"],
                               u_lower=d.get("u_lower"), u_upper=d.get("u_upper"), dma_late=True, layouts=layouts)
    more = {} if qp_start is None else dict(qp_start=qp_start)
    return emu.lqr_step(kernel=kernel, dma_late=True, dtype=dtype, layouts=layouts, **d, **more)


# kernel -> (first fixture: every layout; second: the mixed ones).  A builder returns (kw, with a qp_start?)
def _masked_12_4():
    return cut(golden("step_masked_nc4_f32"), 6), False


def _box_12_4():
    return cut(golden("step_ns_bounded_f32"), 6), True


def _cfg5():
    return cut(golden("step_cfg5_f32"), 5), False


CASES = {
    "dpp16": (_masked_12_4, _box_12_4),
    "dpp16_ring2": (_masked_12_4, _box_12_4),
    "dpp16_pad": (lambda: (random_case(7, 3, 5, 3, 73, bounds=0.4), False), lambda: (cut(golden("step_ns_bounded_f32"), 5, 3), False)),
    "mfma16": (lambda: (cut(golden("step_cfg1_f32"), 5, 5), False), lambda: (random_case(7, 3, 4, 3, 74), False)),
    "mfma16_f64": (lambda: (cut(golden("step_cfg1_f64"), 5, 5), False), lambda: (cut(golden("step_ns_bounded_f64"), 4, 2), False)),
    "mfma40": (_cfg5, lambda: (random_case(32, 8, 4, 3, 328, bounds=0.4), True)),
    "mfma40_ring2": (_cfg5, lambda: (random_case(32, 8, 4, 3, 328, bounds=0.4), True)),
    "mfma40_pad4": (lambda: (random_case(13, 4, 4, 3, 134), False), lambda: (random_case(20, 4, 4, 3, 204, bounds=0.4), True)),
    "mfma40_pad16": (lambda: (random_case(24, 8, 4, 3, 248), False), lambda: (random_case(20, 4, 4, 3, 204, bounds=0.4), True)),
    "narrow4": (lambda: (random_case(13, 4, 4, 3, 134), False), lambda: (random_case(16, 4, 4, 3, 164, bounds=0.4), False)),
    "narrow16": (lambda: (random_case(16, 4, 4, 3, 164), False), lambda: (random_case(16, 4, 4, 3, 164, bounds=0.4), False)),
    "tiny": (lambda: (cut(golden("step_nc1_unbounded_f32"), 6), False), lambda: (cut(golden("step_nc1_bounded_f32"), 5), False)),
    "tiny_f64": (lambda: (cut(golden("step_nc1_scalar_f64"), 6), False), None),
    "wave1": (lambda: (cut(golden("step_nc1_unbounded_f32"), 6), False), lambda: (cut(golden("step_nc1_bounded_f32"), 5), False)),
}
STEP_PARAMS = [(kernel, which, layout) for kernel, pair in CASES.items() for which in (0, 1) if pair[which] is not None
               for layout in (SV.LAYOUTS if which == 0 else tuple(SV.MIXED) + (("pitch_off",) if kernel == "dpp16_pad" else ()))]


@pytest.mark.parametrize("kernel,which,layout", STEP_PARAMS, ids=["%s-%d-%s" % p for p in STEP_PARAMS])
def test_emulated_step_on_views(emu, kernel, which, layout):
    kw, hint = CASES[kernel][which]()
    if not admitted(kernel, layout, kw):
        # refused by the kernel's rule on the device (tests/test_stride_rules_host.py, tests/test_gpu_strided.py): nothing to emulate
        assert layout == "pitch_off"
        return
    dtype = np.float64 if kernel.endswith("_f64") else np.float32
    name = kernel[:-4] if kernel.endswith("_f64") else kernel
    d = shown(kw, layout)
    qp = None
    if hint:
        T, B, nc = d["cur_u"].shape
        qp = np.random.default_rng(5).uniform(-0.4, 0.4, (T, B, nc)).astype(np.float32)
    r = run_step(emu, name, d, layout, qp, dtype)
    dense = run_step(emu, name, d, None, qp, dtype)
    bitwise(r, dense, STEP_OUT, "%s under %s" % (kernel, layout))
    assert np.isfinite(r["new_x"]).all() and np.isfinite(r["new_u"]).all() and np.isfinite(r["K"]).all() and np.isfinite(r["k"]).all()
    hold_step(r, oracle_step(d), d)


# ---------------------------------------------------------------------------------------------
# the KKT backward: kkt_wave (gradients alone) and the fused kernels, exact and padded
# ---------------------------------------------------------------------------------------------
def kkt_case(ns, nc, T, B, seed, layout, bounded):
    """The recipe of test_emulated_fused_kkt_backward_matches_oracle on the values the layout shows: a few oracle steps to the
    solution the backward differentiates at, rounded to float32, and the oracle's three-stage backward there."""
    from oracle import lqr_oracle as O
    d = shown(random_case(ns, nc, T, B, seed), layout)
    pr = {k: f64(d[k]) for k in ("C", "c", "F", "f", "x_init")}
    pr["C"] = pr["C"] + 0.4 * np.eye(ns + nc)
    pr["C"] = pr["C"].astype(np.float32).astype(np.float64)
    lo, hi = (-0.4, 0.4) if bounded else (None, None)
    x, u = f64(d["cur_x"]), f64(d["cur_u"])
    for _ in range(4):
        sol = O.lqr_step(lockstep=False, cur_x=x, cur_u=u, u_lower=lo, u_upper=hi, **pr)
        x, u = sol["new_x"], sol["new_u"]
    x, u = x.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(seed + 1)
    dl_dx, dl_du = rng.standard_normal((T, B, ns)), rng.standard_normal((T, B, nc))
    o = O.kkt_backward(pr["C"], pr["c"], pr["F"], pr["f"], x, u, dl_dx, dl_du, lo, hi, lockstep=False)
    return pr, x, u, dl_dx, dl_du, lo, hi, o


def hold_grads(r, o, keys, wide):
    for k in keys:
        if o[k] is None or o[k].size == 0:
            continue
        assert np.isfinite(r[k]).all(), k
        np.testing.assert_allclose(r[k], o[k], rtol=1e-4 * wide, atol=1e-4 * wide * max(1.0, np.abs(o[k]).max()), err_msg=k)


KKT_KERNELS = {"kkt_grads": (12, 4, True), "fused_dpp16": (12, 4, True), "fused_dpp16_pad": (7, 3, False),
               "fused_mfma40": (32, 8, True), "fused_mfma40_pad4": (13, 4, False), "fused_mfma40_pad16": (16, 4, "gathers")}
KKT_PARAMS = [(k, l) for k in KKT_KERNELS for l in SV.LAYOUTS]


@pytest.mark.parametrize("kernel,layout", KKT_PARAMS, ids=["%s-%s" % p for p in KKT_PARAMS])
def test_emulated_kkt_backward_on_views(emu, kernel, layout):
    ns, nc, grid = KKT_KERNELS[kernel]
    T, B = 5, 3
    bounded = layout in ("mixed_a", "pitch_grid", "shared_b", "batch_major")
    pr, x, u, dl_dx, dl_du, lo, hi, o = kkt_case(ns, nc, T, B, 40 + ns, layout, bounded)
    if grid:
        # (the KKT rules ask the grid of C, c and F; the gathers of C and F)
        pl = SV.place_problem(layout, np, pr["C"].astype(np.float32), pr["c"].astype(np.float32), pr["F"].astype(np.float32))
        if not SV.on_grid({r: pl[r] for r in (("C", "F") if grid == "gathers" else ("C", "c", "F"))}, 4):
            assert layout == "pitch_off"
            return
    keys = ("dx", "du", "dC", "dc", "dF", "dx_init", "df")
    if kernel == "kkt_grads":
        run = lambda layouts: emu.kkt_grads(pr["C"], pr["c"], pr["F"], pr["f"], x, u, o["dx"], o["du"], dl_dx, dma_late=True, ring2=True, layouts=layouts)
        keys, wide = ("dC", "dc", "dF", "dx_init", "df"), 1.0
    elif kernel.startswith("fused_dpp16"):
        run = lambda layouts: emu.kkt_fused(pr["C"], pr["c"], pr["F"], pr["f"], x, u, dl_dx, dl_du, lo, hi, dma_late=True,
                                            kernel="dpp16_pad" if kernel.endswith("pad") else "dpp16", layouts=layouts)
        wide = 1.0
    else:
        pad = int(kernel[len("fused_mfma40_pad"):]) if "pad" in kernel else 0
        run = lambda layouts: emu.kkt_fused_mfma40(pr["C"], pr["c"], pr["F"], pr["f"], x, u, dl_dx, dl_du, lo, hi, dma_late=True, pad=pad, layouts=layouts)
        wide = 2.0
    r, dense = run(layout), run(None)
    bitwise(r, dense, keys, "%s under %s" % (kernel, layout))
    hold_grads(r, o, keys, wide)


# ---------------------------------------------------------------------------------------------
# the row-per-problem kernel's carry instantiation (tests/emu_row_carry.py): C, c and the caller's augmented F as views
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", SV.LAYOUTS)
@pytest.mark.parametrize("linearize", [False, True], ids=["F-given", "linearize"])
@pytest.mark.parametrize("kind", ["pendulum", "cartpole"])
def test_emulated_carry_body_on_views(kind, linearize, layout):
    """Bitwise against the same body on the dense copy of the values the views show (the nominal obeys the simulator, not F, so it
    stays); test_emu_row_carry.py holds the dense call to the lane-per-problem body."""
    import test_emu_row_carry as RC
    k = RC.case(kind)
    pl = SV.place_problem(layout, np, k["C"], k["c"], k["F"])
    d = dict(k, C=pl["C"].dense, c=pl["c"].dense, F=pl["F"].dense)

    def run(layouts):
        rc, out = RC.R.step(d["kind"], d["params"], d["dt"], d["u_max"], d["x_init"], d["C"], d["c"], None if linearize else d["F"], d["cur_x"],
                            d["cur_u"], -RC.BOUND, RC.BOUND, max_linesearch_iter=10, linesearch_decay=d["decay"], layouts=layouts)
        assert rc == 0, rc
        return out
    r, dense = run(layout), run(None)
    bitwise(r, dense, STEP_OUT, "carry body (%s) under %s" % (kind, layout))
    assert np.isfinite(r["new_x"]).all() and np.isfinite(r["new_u"]).all() and np.isfinite(r["costs"]).all()
