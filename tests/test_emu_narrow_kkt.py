"""The fused KKT backward of the NARROW instantiation (lqr_mfma40_body.h: kkt_fused_wave with -DMPC_MFMA40_XT=1, the library's
lqr_mfma40_narrow4kkt.o / _narrow16kkt.o) through the unchanged wavefront emulator: pass 2's workspace is PACKED at one state tile
(V_t 256 words a problem-step, fetched once; v_t | g_t 16 + 16 words; four + four record lanes), and every output must still be the
float64 oracle's within the padded kernel's own emulator tolerances AND the padded emulator library's bit for bit (the second state
tile holds exact zeros at these shapes; the emulator is built with contraction off).  The emulator hands the body pointers into an
allocation sized for the two-tile layout, so the packed strides stay inside it.  Outputs are pre-filled with NaN by the driver: an
entry the kernel skips fails."""
import numpy as np
import pytest

import emu_backend as E
import emu_narrow as EN

CASES = ["16_4", "13_4_bounded", "16_8_tensor", "14_3_T1", "16_4_T2_bounded", "9_6_nof", "1_1", "16_4_nof", "13_1", "14_2_nonconvex", "2_5",
         "16_4_T3"]


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


def _same_bits(a, b):
    """equal bit for bit, +0 and -0 alike"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))).all())


def _narrow(pad, *args, **kw):
    """emu_backend.kkt_fused_mfma40's driver on the narrow emulator library of this gather granule (the driver takes its library from
    emu_backend.lib_pad and offers no other hook)"""
    padded = E.lib_pad
    E.lib_pad = lambda p: EN.lib(p)
    try:
        return E.kkt_fused_mfma40(*args, pad=pad, **kw)
    finally:
        E.lib_pad = padded


@pytest.mark.parametrize("case", CASES)
def test_emulated_narrow_fused_kkt_backward_matches_oracle_and_the_padded_library_bitwise(case):
    from oracle import lqr_oracle as O
    parts = case.split("_")
    ns, nc = int(parts[0]), int(parts[1])
    rng = np.random.default_rng(sum(map(ord, case)) + 7)
    T = next((int(q[1:]) for q in parts[2:] if q[0] == "T"), 5)
    B = 3
    bounded = "bounded" in parts or "tensor" in parts
    pr = _shape_problem(rng, max(T, 2), B, ns, nc, with_f="nof" not in parts)
    if "nonconvex" in parts:
        pr["C"][:, (0, 2), ns:, ns:] -= 400.0 * np.eye(nc)
    if T == 1:
        pr = {k: (v[:1] if k in ("C", "c") else (v[:0] if k in ("F", "f") and v is not None else v)) for k, v in pr.items()}
    cur_u = np.clip(0.5 * rng.standard_normal((T, B, nc)), -0.4, 0.4)
    cur_x, _ = O.traj_cost(pr["x_init"], cur_u, pr["F"], pr["f"])
    lo, hi = (-0.4, 0.4) if bounded else (None, None)
    if "tensor" in parts:
        lo, hi = -0.3 - 0.2 * rng.random((T, B, nc)), 0.3 + 0.2 * rng.random((T, B, nc))
        lo, hi = lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)
    x, u = cur_x, cur_u
    for _ in range(4):
        sol = O.lqr_step(lockstep=False, cur_x=x, cur_u=u, u_lower=lo, u_upper=hi, **pr)
        x, u = sol["new_x"], sol["new_u"]
    x, u = x.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)
    dl_dx, dl_du = rng.standard_normal((T, B, ns)), rng.standard_normal((T, B, nc))
    o = O.kkt_backward(pr["C"], pr["c"], pr["F"], pr["f"], x, u, dl_dx, dl_du, lo, hi, lockstep=False)
    if bounded and T > 2:
        act = np.abs(np.abs(u) - 0.4) <= 1e-8 if "tensor" not in parts else (np.abs(u - lo) <= 1e-8) | (np.abs(u - hi) <= 1e-8)
        assert 0.01 < act.mean() < 0.97, act.mean()
    args = (pr["C"], pr["c"], pr["F"], pr["f"], x, u, dl_dx, dl_du, lo, hi)
    for dma_late, pad in ((False, 4), (True, 4)) + (((False, 16), (True, 16)) if ns % 4 == 0 and nc % 4 == 0 else ()):
        r = _narrow(pad, *args, dma_late=dma_late)
        wide = 20.0 if "nonconvex" in parts else 2.0
        for k in ("dx", "du", "dC", "dc", "dF", "dx_init") + (("df",) if pr["f"] is not None and T > 1 else ()):
            if o[k] is None or o[k].size == 0:
                continue
            assert np.isfinite(r[k]).all(), (k, dma_late, pad)
            np.testing.assert_allclose(r[k], o[k], rtol=1e-4 * wide, atol=1e-4 * wide * max(1.0, np.abs(o[k]).max()), err_msg="%s %s %s" % (k, dma_late, pad))
        rp = E.kkt_fused_mfma40(*args, dma_late=dma_late, pad=pad)
        for k in ("dx", "du", "dx_init", "dC", "dc") + (("dF", "lam1", "dlam1") if T > 1 else ()) + (("df",) if r["df"] is not None and T > 1 else ()):
            assert _same_bits(r[k], rp[k]), (k, dma_late, pad, np.abs(r[k].astype(np.float64) - rp[k]).max())


# ---------------------------------------------------------------------------------------------
# Horizons past pass 2's three-slot ring, under every combination of the emulator's switches (docs/history/r24.md): the DMA landing
# at issue or at the covering wait, its source read at issue or at landing, the wave's own stores visible at once or at the fence,
# an LDS-DMA that no lane takes part in counted or not.  A correct kernel gives identical bits under all sixteen.
# ---------------------------------------------------------------------------------------------
KSLOTS = 3                                   # lqr_mfma40_body.h
MODELS = [(late, model) for late in (False, True) for model in range(8)]
CORNERS = [(False, 0), (True, 0), (False, 7), (True, 7)]      # T = 70: seventy timesteps a run; every switch off / on, with either landing time
LONG = ["16_4_T%d_bounded" % (2 * KSLOTS + 1), "13_4_T%d_bounded" % (2 * KSLOTS + 1), "16_4_T%d" % (2 * KSLOTS + 1),
        "12_4_T%d_tensor" % (2 * KSLOTS + 1), "16_4_T70_B1_bounded"]


def _long_problem(case):
    """the recipe of the test above at the case's horizon and batch -> (arguments of the drivers, the oracle's backward, T)"""
    from oracle import lqr_oracle as O
    parts = case.split("_")
    ns, nc = int(parts[0]), int(parts[1])
    rng = np.random.default_rng(sum(map(ord, case)) + 11)
    T = next(int(q[1:]) for q in parts[2:] if q[0] == "T")
    B = next((int(q[1:]) for q in parts[2:] if q[0] == "B"), 3)
    pr = _shape_problem(rng, T, B, ns, nc)
    cur_u = np.clip(0.5 * rng.standard_normal((T, B, nc)), -0.4, 0.4)
    cur_x, _ = O.traj_cost(pr["x_init"], cur_u, pr["F"], pr["f"])
    lo, hi = (-0.4, 0.4) if "bounded" in parts else (None, None)
    if "tensor" in parts:
        lo, hi = -0.3 - 0.2 * rng.random((T, B, nc)), 0.3 + 0.2 * rng.random((T, B, nc))
        lo, hi = lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)
    x, u = cur_x, cur_u
    for _ in range(4):
        sol = O.lqr_step(lockstep=False, cur_x=x, cur_u=u, u_lower=lo, u_upper=hi, **pr)
        x, u = sol["new_x"], sol["new_u"]
    x, u = x.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)
    dl_dx, dl_du = rng.standard_normal((T, B, ns)), rng.standard_normal((T, B, nc))
    o = O.kkt_backward(pr["C"], pr["c"], pr["F"], pr["f"], x, u, dl_dx, dl_du, lo, hi, lockstep=False)
    return (pr["C"], pr["c"], pr["F"], pr["f"], x, u, dl_dx, dl_du, lo, hi), o, (ns, nc, T)


def _models(T):
    return MODELS if T < 70 else CORNERS


def _identical_under_every_model(run, o, keys, what, models=MODELS):
    """run(dma_late, model) -> outputs; the plain emulator's are held to the oracle (the tolerance of the test above), every other
    combination's to the plain emulator's, bit for bit, NaN for NaN"""
    base = run(False, 0)
    for k in keys:
        assert np.isfinite(base[k]).all(), (what, k)
        np.testing.assert_allclose(base[k], o[k], rtol=2e-4, atol=2e-4 * max(1.0, np.abs(o[k]).max()), err_msg="%s %s" % (what, k))
    for late, model in models[1:]:
        r = run(late, model)
        for k in keys:
            a, b = np.ascontiguousarray(r[k]).view(np.uint32), np.ascontiguousarray(base[k]).view(np.uint32)
            assert np.array_equal(a, b), "%s %s: dma_late %d, model %d (1 source at landing | 2 own stores late | 4 idle DMAs not counted) " \
                "differs from the plain emulator in %d words, first at %s" % (what, k, late, model, int((a != b).sum()), np.argwhere(a != b)[0].tolist())


KEYS = ("dx", "du", "dx_init", "dC", "dc", "dF", "df")


@pytest.mark.parametrize("case", LONG)
def test_emulated_narrow_fused_kkt_backward_is_the_same_under_every_switch_of_the_emulator(case):
    args, o, (ns, nc, T) = _long_problem(case)
    for pad in ((4,) if T < 70 else ()) + ((16,) if ns % 4 == 0 and nc % 4 == 0 else ()):
        _identical_under_every_model(lambda late, model: _narrow(pad, *args, dma_late=late, model=model), o, KEYS, "narrow pad %d" % pad, _models(T))


@pytest.mark.parametrize("case", LONG)
def test_emulated_padded_fused_kkt_backward_is_the_same_under_every_switch_of_the_emulator(case):
    """the two-tile padded library on the same problems"""
    args, o, (ns, nc, T) = _long_problem(case)
    for pad in ((4,) if T < 70 else ()) + ((16,) if ns % 4 == 0 and nc % 4 == 0 else ()):
        _identical_under_every_model(lambda late, model: E.kkt_fused_mfma40(*args, dma_late=late, pad=pad, model=model), o, KEYS, "padded pad %d" % pad,
                                     _models(T))


@pytest.mark.parametrize("case", ["12_4_T%d_bounded" % (2 * KSLOTS + 1), "12_4_T%d" % (2 * KSLOTS + 1), "12_4_T%d_tensor" % (2 * KSLOTS + 1),
                                  "12_4_T70_B4_bounded"])
def test_emulated_12_4_fused_kkt_backward_is_the_same_under_every_switch_of_the_emulator(case):
    """E.kkt_fused: kkt_fused_wave of lqr_dpp16_body.h, four problems a wavefront, both horizon modes (T = 70: the record beyond 64 steps)"""
    args, o, (_, _, T) = _long_problem(case)
    _identical_under_every_model(lambda late, model: E.kkt_fused(*args, dma_late=late, model=model), o, KEYS, "12/4", _models(T))


@pytest.mark.parametrize("case", ["16_4_T%d_bounded" % (2 * KSLOTS + 1), "13_4_T%d" % (2 * KSLOTS + 1)])
@pytest.mark.parametrize("vouched", [False, True], ids=["bare", "vouched"])
def test_emulated_narrow_step_is_the_same_under_every_switch_of_the_emulator(case, vouched):
    """the one-tile STEP kernel (impl 9) on the same problems, from the point the backward was taken at: its sweep stages the same
    record, and its rollouts read the parked gains back through the ring"""
    (C, c, F, f, x, u, _, _, lo, hi), _, (ns, nc, T) = _long_problem(case)
    keys = ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alpha_du_norm", "alphas", "K", "k")
    for pad in (4,) + ((16,) if ns % 4 == 0 and nc % 4 == 0 else ()):
        run = lambda late, model: EN.step(EN.lib(pad), x[0], C, c, F, f, x, u, u_lower=lo, u_upper=hi, nominal_on_dynamics=vouched,
                                          c_symmetric=vouched, dma_late=late, model=model)
        base = run(False, 0)
        for k in keys[:7]:
            assert np.isfinite(base[k]).all(), (k, pad)
        for late, model in MODELS[1:]:
            r = run(late, model)
            for k in keys:
                a, b = np.ascontiguousarray(r[k]).view(np.uint32), np.ascontiguousarray(base[k]).view(np.uint32)
                assert np.array_equal(a, b), "pad %d %s: dma_late %d, model %d differs from the plain emulator in %d words" % (pad, k, late, model, int((a != b).sum()))
