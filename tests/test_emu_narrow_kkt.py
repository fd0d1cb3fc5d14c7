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
