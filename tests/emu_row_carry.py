"""TEST INFRASTRUCTURE: the CARRY instantiation of the row-per-problem kernel (lqr_wave1_body.h with -DMPC_WAVE1_CARRY: a shipped
simulator behind MPC_ENV_CTRL_CARRY, n_state = 4 / 6, impl 10) on the CPU, through the unchanged wavefront emulator
tests/emu/emu_mfma16.cpp -- compiled into a library of its own name with emu_backend.build's plain command plus the macro -- and the
driver that runs its emu_lqr_step_wave1 on one float32 problem."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import emu_backend as E
from mpc import _native as N

_LIB = None


def build():
    """emu_backend.build()'s compiler line plus -DMPC_WAVE1_CARRY, into a library of its own name.  (That function takes no further
    flags and offers no hook, so its line is repeated here, as tests/emu_narrow.py does.)"""
    so = os.path.join(E._EMU, "libemu_mfma16_row_carry.so")
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
                subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-DMPC_WAVE1_CARRY", "-o", tmp, src])
                os.replace(tmp, so)
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        _LIB.emu_lqr_step_wave1.argtypes = [ctypes.POINTER(N.Problem), ctypes.POINTER(N.Options), ctypes.POINTER(N.Outputs)]
    return _LIB


def step(kind, params, dt, u_max, x_init, C, c, F, cur_x, cur_u, lo, hi, max_linesearch_iter=10, linesearch_decay=0.2, carry=True, layouts=None):
    """One step of the emulated row-per-problem carry body: z = (u_prev, x) [B, ns + 1], C [T, B, n, n], scalar bounds, the simulator
    `kind` (MPC_ENV_*) behind the carry as true dynamics; F = None: the body linearises the simulator itself, else the caller's
    augmented F [T-1, B, ns + 1, ns + 2] is the sweep's model.  Returns (rc, outputs): rc != 0 is the body's refusal."""
    f32 = np.float32
    C = np.ascontiguousarray(C, f32); c = np.ascontiguousarray(c, f32); x_init = np.ascontiguousarray(x_init, f32)
    cur_x = np.ascontiguousarray(cur_x, f32); cur_u = np.ascontiguousarray(cur_u, f32)
    T, B, n, _ = C.shape
    ns = x_init.shape[1]
    assert n == ns + 1
    keep = []
    p = N.Problem()
    p.B, p.T, p.ns, p.nc, p.dtype = B, T, ns, 1, N.MPC_F32
    p.x_init = E._ptr(x_init)
    p.C, p.C_st, p.C_sb = E._ptr(C), B * n * n, n * n
    p.c, p.c_st, p.c_sb = E._ptr(c), B * n, n
    if F is not None and T > 1:
        F = np.ascontiguousarray(F, f32)
        p.F, p.F_st, p.F_sb = E._ptr(F), B * ns * n, ns * n
    p.cur_x, p.cur_u = E._ptr(cur_x), E._ptr(cur_u)
    o = N.Options()
    o.max_linesearch_iter, o.linesearch_decay, o.pnqp_iter = int(max_linesearch_iter), float(linesearch_decay), 20
    o.delta_u = float("nan")
    o.bound_mode, o.lo_s, o.hi_s = N.BOUND_SCALAR, float(lo), float(hi)
    if kind:
        e = N.EnvDynamics()
        prm = np.ascontiguousarray(params, f32)
        keep.append(prm)
        e.kind = int(kind) | (N.ENV_CTRL_CARRY if carry else 0)
        e.params, e.dt, e.u_max, e.linearize = E._ptr(prm), float(dt), float(u_max), int(F is None)
        keep.append(e)
        o.true_dynamics = ctypes.pointer(e)
    if layouts is not None:          # (a row of tests/strided_views.py's table; None: the dense layout as ever)
        E.place_views(p, layouts, keep, C, c, F if (F is not None and T > 1) else None)
    res = dict(new_x=np.full((T, B, ns), np.nan, f32), new_u=np.full((T, B, 1), np.nan, f32),
               costs=np.full(B, np.nan, f32), old_costs=np.full(B, np.nan, f32), full_du_norm=np.full(B, np.nan, f32),
               alpha_du_norm=np.full(B, np.nan, f32), alphas=np.full(B, np.nan, f32),
               qp_iters=np.zeros(B, np.int32), status=np.zeros(B, np.int32),
               K=np.full((T, B, 1, ns), np.nan, f32), k=np.full((T, B, 1), np.nan, f32))
    out = N.Outputs()
    for key, arr in res.items():
        setattr(out, key, E._ptr(arr))
    rc = lib().emu_lqr_step_wave1(ctypes.byref(p), ctypes.byref(o), ctypes.byref(out))
    return rc, res
