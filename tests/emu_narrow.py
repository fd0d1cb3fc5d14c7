"""TEST INFRASTRUCTURE: the NARROW instantiation of the 32/8 kernel (lqr_mfma40_body.h with -DMPC_MFMA40_XT=1: one 16-row state
tile, n_state <= 16) on the CPU, through the unchanged wavefront emulator tests/emu/emu_mfma16.cpp -- compiled into libraries of
their own names with emu_backend.build's command for pad = 4 | 16 plus -DMPC_MFMA40_XT=1 -- and the driver that runs
emu_lqr_sweep_mfma40 of any emulator library on one problem (the padded libraries of emu_backend among them)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import emu_backend as E
from mpc import _native as N

_LIBS = {}


def build(pad):
    """emu_backend.build(pad=pad)'s compiler line plus -DMPC_MFMA40_XT=1, into a library of its own name.  (That function
    takes no further flags and offers no hook, so its line is repeated here; tests/test_emu_narrow.py holds the two lines together.)
    The two-slot sweep ring is that recipe's; the library's narrow objects sweep on three slots, which the device tests cover."""
    assert pad in (4, 16)
    so = os.path.join(E._EMU, "libemu_mfma16_narrow%d.so" % pad)
    src = os.path.join(E._EMU, "emu_mfma16.cpp")
    csrc = os.path.join(E._HERE, "..", "mpc.pytorch_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("lqr_mfma16_body.h", "lqr_dpp16_body.h", "lqr_small_math.h", "lqr_params.h",
                                                    "env_dynamics.h", "lqr_tiny_body.h", "lqr_wave1_body.h", "lqr_mfma40_body.h")]

    def stale():
        return not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps)
    if stale():
        import fcntl
        with open(so + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                cxx = "/opt/rocm/lib/llvm/bin/clang++"
                if not os.path.exists(cxx):
                    cxx = shutil.which("clang++")
                assert cxx, "the emulator needs clang++ (ext_vector_type)"
                tmp = so + ".tmp%d" % os.getpid()
                subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                                       "-DMPC_DPP16_NSTAGE=2", "-DMPC_KKT16_NSTAGE=2", "-DMPC_MFMA40_SWEEP_NSTAGE=2",
                                       "-DMPC_MFMA40_PAD=%d" % pad, "-DMPC_DPP16_PAD", "-DMPC_KF_LDS_BYTES=36864",
                                       "-DMPC_MFMA40_XT=1", "-o", tmp, src])
                os.replace(tmp, so)
    return so


def lib(pad):
    if pad not in _LIBS:
        _LIBS[pad] = ctypes.CDLL(build(pad))
    return _LIBS[pad]


def step(L, x_init, C, c, F, f, cur_x, cur_u, full=True, u_lower=None, u_upper=None, u_zero_I=None, delta_u=None,
         nominal_on_dynamics=False, c_symmetric=False, max_linesearch_iter=10, linesearch_decay=0.2, pnqp_iter=20, dma_late=False, model=0, layouts=None):
    """emu_lqr_sweep_mfma40 of the emulator library L (full: the whole step; else the sweep alone) on one float32 problem.
    Returns every output, the caller's K / k among them.  dma_late, model: the emulator's switches (emu_backend.MODEL_*)."""
    f32 = np.float32
    C = np.ascontiguousarray(C, f32); c = np.ascontiguousarray(c, f32); x_init = np.ascontiguousarray(x_init, f32)
    T, B, n, _ = C.shape
    ns = x_init.shape[1]
    nc = n - ns
    F = np.ascontiguousarray(F, f32) if T > 1 else np.zeros((0, B, ns, n), f32)
    f = None if (f is None or np.asarray(f).size == 0) else np.ascontiguousarray(f, f32)
    cur_x = np.ascontiguousarray(cur_x, f32); cur_u = np.ascontiguousarray(cur_u, f32)
    p = N.Problem()
    p.B, p.T, p.ns, p.nc, p.dtype = B, T, ns, nc, N.MPC_F32
    p.x_init = E._ptr(x_init)
    p.C, p.C_st, p.C_sb = E._ptr(C), B * n * n, n * n
    p.c, p.c_st, p.c_sb = E._ptr(c), B * n, n
    if T > 1:
        p.F, p.F_st, p.F_sb = E._ptr(F), B * ns * n, ns * n
    if f is not None:
        p.f, p.f_st, p.f_sb = E._ptr(f), B * ns, ns
    p.cur_x, p.cur_u = E._ptr(cur_x), E._ptr(cur_u)
    o = N.Options()
    o.max_linesearch_iter, o.linesearch_decay, o.pnqp_iter = int(max_linesearch_iter), float(linesearch_decay), int(pnqp_iter)
    o.delta_u = float("nan") if delta_u is None else float(delta_u)
    o.flags = (N.OPT_NOMINAL_ON_DYNAMICS if nominal_on_dynamics else 0) | (N.OPT_C_SYMMETRIC if c_symmetric else 0)
    keep = []
    if u_lower is None:
        o.bound_mode = N.BOUND_NONE
    elif isinstance(u_lower, float) and isinstance(u_upper, float):
        o.bound_mode, o.lo_s, o.hi_s = N.BOUND_SCALAR, u_lower, u_upper
    else:
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(u_lower, f32), (T, B, nc)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(u_upper, f32), (T, B, nc)))
        keep += [lo, hi]
        o.bound_mode, o.lo, o.hi = N.BOUND_TENSOR, E._ptr(lo), E._ptr(hi)
    if u_zero_I is not None:
        zm = np.ascontiguousarray((np.asarray(u_zero_I) != 0).astype(np.uint8))
        keep.append(zm)
        o.zero_mask = E._ptr(zm)
    if layouts is not None:          # (a row of tests/strided_views.py's table; None: the dense layout as ever)
        E.place_views(p, layouts, keep, C, c, F, f)
    res = dict(new_x=np.full((T, B, ns), np.nan, f32), new_u=np.full((T, B, nc), np.nan, f32),
               costs=np.full(B, np.nan, f32), old_costs=np.full(B, np.nan, f32), full_du_norm=np.full(B, np.nan, f32),
               alpha_du_norm=np.full(B, np.nan, f32), alphas=np.full(B, np.nan, f32),
               qp_iters=np.zeros(B, np.int32), status=np.zeros(B, np.int32),
               K=np.full((T, B, nc, ns), np.nan, f32), k=np.full((T, B, nc), np.nan, f32))
    out = N.Outputs()
    for key, arr in res.items():
        setattr(out, key, E._ptr(arr))
    L.emu_set_dma_late(int(bool(dma_late)))
    L.emu_set_model(int(model))
    L.emu_mfma40_full(int(bool(full)))
    fn = L.emu_lqr_sweep_mfma40
    fn.argtypes = [ctypes.POINTER(N.Problem), ctypes.POINTER(N.Options), ctypes.POINTER(N.Outputs)]
    try:
        rc = fn(ctypes.byref(p), ctypes.byref(o), ctypes.byref(out))
    finally:
        L.emu_set_dma_late(0)
        L.emu_set_model(0)
    assert rc == 0, rc
    return res
