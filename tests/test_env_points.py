"""CPU tests of tests/env_points.py: the stratified points the simulator kernels are held to float64 on
(tests/test_gpu_env_points.py), their input conditions, and c_host -- the error of env_dynamics.h's HOST build (libm, IEEE
division; tests/emu_backend.env_linearize) in env_points' unit.  c_host is the yardstick for what the number format can do on
these points; it says nothing about the device's fast paths, which no CPU test runs.

c_host as measured here (env_points.C_HOST holds these figures, rounded up in the last digit):

    kind           stratum   float64: next     F         f        float32: next     F         f
    pendulum       fixture            2.1e-16  2.1e-16  1.9e-15           7.2e-08  1.1e-07  1.5e-07
    pendulum       fast               1.1e-16  1.0e-16  8.2e-16           8.3e-08  7.6e-08  7.9e-07
    pendulum       edge32             1.1e-16  9.0e-17  2.5e-15           8.7e-08  7.9e-08  1.0e-06
    pendulum       past               7.7e-17  7.5e-17  4.1e-15           8.1e-08  8.3e-08  6.3e-06
    pendulum       far                9.2e-17  8.6e-17  1.1e-14           8.3e-08  7.8e-08  1.1e-05
    pendulum       radius             7.3e-16  3.6e-15  1.4e-15           2.3e-07  6.0e-07  1.6e-06
    pendulum_full  fixture            7.3e-17  9.6e-17  1.2e-16           5.0e-08  7.0e-08  2.4e-07
    pendulum_full  fast               0.0e+00  2.8e-17  3.6e-17           9.4e-08  8.4e-08  1.1e-06
    pendulum_full  edge32             0.0e+00  4.2e-18  5.7e-18           1.1e-07  9.1e-08  3.1e-06
    pendulum_full  past               0.0e+00  2.0e-18  2.7e-18           1.1e-07  9.8e-08  3.7e-06
    pendulum_full  far                0.0e+00  3.8e-20  0.0e+00           9.4e-08  9.2e-08  7.1e-06
    pendulum_full  radius             5.2e-17  2.5e-16  9.4e-17           5.9e-08  4.0e-06  1.3e-07
    cartpole       fixture            6.0e-16  2.7e-16  1.5e-15           5.1e-07  1.4e-07  1.5e-07
    cartpole       fast               2.8e-15  1.9e-16  1.5e-15           3.4e-07  5.7e-08  6.8e-07
    cartpole       edge32             2.4e-16  9.0e-17  1.3e-15           2.4e-07  5.7e-08  1.5e-06
    cartpole       past               9.8e-17  9.8e-17  9.1e-15           6.3e-08  5.1e-08  2.3e-06
    cartpole       far                9.7e-17  8.4e-17  8.9e-14           6.8e-08  6.3e-08  6.9e-05
    cartpole       radius             1.0e-14  1.1e-14  2.0e-14           2.9e-05  5.8e-05  5.8e-05

c_host (next state) on the transitions the emulated step kernels return for env_points.step_problem, the largest over tiny (plain,
carry, in-kernel linearisation), wave1 and wave1_carry (env_points.C_HOST_STEP holds these, rounded up in the last digit):

    kind           stratum   float64   float32
    pendulum       fixture   2.9e-16   7.9e-08
    pendulum       fast      1.3e-16   8.1e-08
    pendulum       past      1.9e-16   7.6e-08
    pendulum_full  fixture   8.9e-17   3.7e-08
    pendulum_full  fast      8.5e-17   1.2e-07
    pendulum_full  past      0.0e+00   1.2e-07
    cartpole       fixture   5.9e-16   3.2e-07
    cartpole       fast      1.9e-15   2.1e-06
"""
import numpy as np
import pytest
import torch

from mpc import _native

import env_points as P

DTYPES = (torch.float64, torch.float32)
NP = {torch.float64: np.float64, torch.float32: np.float32}


def host_linearize(emu, kind, x, u, dtype):
    prm = P.params_of(kind, dtype).numpy()
    with np.errstate(all="ignore"):
        return emu.env_linearize(P.KIND_CODE[kind], prm, P.DT, P.u_max_of(kind), x.numpy(), u.numpy(), NP[dtype])


def measure(emu, kind, name, dtype):
    """c_host (next, F, f) of one stratum"""
    x, u = P.stratum(kind, name, dtype)
    nxt, F, f, A = P.reference(kind, x, u)
    sc = P.scales(x.double().numpy(), u.double().numpy(), nxt, F, A)
    got = dict(zip(P.OUTPUTS, host_linearize(emu, kind, x, u, dtype)))
    return tuple(P.c_of(got[o], r, sc[o]) for o, r in zip(P.OUTPUTS, (nxt, F, f)))


@pytest.mark.parametrize("kind", P.KINDS)
def test_host_error_per_stratum(emu_libs, kind):
    """float64: c <= 4 eps64, or the recorded figure where that is higher.  float32: c within HOST_LIBM_MARGIN of the recorded
    figure (the figures move a little with the host's libm; the margin is for this check alone, the device's bounds take the
    table as it is).  Both: the table is not more than twice above the measurement."""
    for name in P.STRATA:
        for dtype, tag in zip(DTYPES, ("f64", "f32")):
            got = measure(emu_libs, kind, name, dtype)
            table = P.C_HOST[kind][name][tag]
            print("c_host %-13s %-7s %s  next %.2e  F %.2e  f %.2e" % ((kind, name, tag) + got))
            for o, g, t in zip(P.OUTPUTS, got, table):
                if dtype == torch.float64:
                    assert g <= max(4 * P.EPS[dtype], t), (kind, name, o, g, t)
                else:
                    assert g <= P.HOST_LIBM_MARGIN * t, (kind, name, o, g, t)
                assert t <= max(2 * g, 4 * P.EPS[dtype]), ("stale table", kind, name, tag, o, g, t)


@pytest.mark.parametrize("kind", P.KINDS)
def test_input_conditions(kind):
    u_max = P.u_max_of(kind)
    iw = 4 if kind == "cartpole" else 2
    ic = 2 if kind == "cartpole" else 0
    w_range = {"fixture": (0, 8), "fast": (40, 600), "edge32": (31.9 / P.DT, 32.1 / P.DT), "past": (700, 5000), "far": (4e4, 1e5),
               "radius": (0, 8)}
    r_range = {"fixture": (0.75, 1.3), "radius": (1e-3, 1e3)}
    for name in P.STRATA:
        for dtype in DTYPES:
            x, u = P.stratum(kind, name, dtype)
            assert x.shape == (P.N, iw + 1) and u.shape == (P.N, 1) and x.dtype == dtype
            outside = int((u.abs() > u_max).sum())
            assert 0.15 * P.N < outside < 0.25 * P.N, (name, outside)
            assert int((u == u_max).sum()) == 1 and int((u == -u_max).sum()) == 1
            w = x[:, iw].double().abs()
            lo, hi = w_range[name]
            slack = 1 + 2 * P.EPS[torch.float32]
            assert float(w.min()) >= lo / slack and float(w.max()) <= hi * slack, (name, float(w.min()), float(w.max()))
            r = x[:, ic:ic + 2].double().norm(dim=1)
            rlo, rhi = r_range.get(name, (1.0, 1.0))
            assert float(r.min()) >= rlo * (1 - 1e-6) and float(r.max()) <= rhi * (1 + 1e-6), (name, float(r.min()), float(r.max()))
            if name == "radius":
                assert float(r.min()) < 1e-2 and float(r.max()) > 1e2
            nxt, F, f, A = P.reference(kind, x, u)
            assert all(np.isfinite(a).all() for a in (nxt, F, f, A)), name
            arg = A - 1
            if name == "fixture":
                assert arg.max() < 4.0
            if name == "fast":
                assert arg.max() > 29.0 and (arg < P.FAST_TRIG_MAX).mean() > 0.9
            if name == "edge32":
                # the float32 product the cart-pole kernel forms, and the float64 argument of every kind: both sides of 32.0f
                prod = (x[:, iw].float() * torch.tensor(P.DT, dtype=torch.float32)).abs()
                assert int((prod <= 32.0).sum()) > 50 and int((prod > 32.0).sum()) > 50
                assert int((arg <= P.FAST_TRIG_MAX).sum()) > 20 and int((arg > P.FAST_TRIG_MAX).sum()) > 20
            if name in ("past", "far"):
                assert arg.min() > P.FAST_TRIG_MAX + 1
            if name == "far":
                assert (arg / (2 * np.pi)).min() > 256
            if kind == "pendulum_full":
                th = np.arctan2(x[:, 1].double().numpy(), x[:, 0].double().numpy())
                assert (np.pi - np.abs(th)).min() > 1e-3


@pytest.mark.parametrize("kind", P.KINDS)
def test_edge_points_on_the_host(emu_libs, kind):
    """float64 host build at the hand-made points: the +-0.0 pair (theta = +pi and -pi: two different successors of the full
    pendulum) and the controls on and beyond the clamp agree with the yardstick; at (0, 0) the transition does (theta = 0
    there).  The Jacobian at (0, 0) is not compared: the header divides by c^2 + s^2."""
    x, u = P.edges(kind)
    nxt, F, f, A = P.reference(kind, x, u)
    keep = np.arange(len(P.EDGE_NAMES)) != P.EDGE_ORIGIN
    assert all(np.isfinite(a[keep]).all() for a in (nxt, F, f)) and np.isfinite(nxt).all()
    sc = P.scales(x.numpy(), u.numpy(), nxt, F, A)
    got = dict(zip(P.OUTPUTS, host_linearize(emu_libs, kind, x, u, torch.float64)))
    tol = 4 * P.EPS[torch.float64]
    assert P.c_of(got["next"], nxt, sc["next"]) <= tol
    ns = x.shape[1]
    # (f = next - F tau sums ns + 2 terms, each with an error of its own of that size)
    for o, r, t in (("F", F, tol), ("f", f, tol * (ns + 2))):
        assert P.c_of(got[o], r, sc[o], keep) <= t, o
    assert (got["F"][list(P.EDGE_BEYOND), :, ns] == 0).all() and (F[list(P.EDGE_BEYOND), :, ns] == 0).all()
    rows = P.U_FREE_ROWS[kind]
    assert np.array_equal(got["F"][list(P.EDGE_ON_CLAMP)][:, rows, ns], got["F"][[P.EDGE_INTERIOR] * 2][:, rows, ns])
    assert (got["F"][P.EDGE_INTERIOR, rows, ns] != 0).all()
    if kind == "pendulum_full":
        a, b = P.EDGE_PI
        assert np.abs(nxt[a] - nxt[b]).max() > 0.09, "dw = dt d 2 pi = 0.094 through the damping term"
        assert np.abs(got["next"][a] - got["next"][b]).max() > 0.09


# the step kernels whose bodies the emulator builds: (emulator kernel, dtypes, carry, in-kernel linearisation)
EMU_STEPS = {"tiny": ("tiny", DTYPES, False, False), "tiny_carry": ("tiny", DTYPES, True, False), "tiny_linearize": ("tiny", DTYPES, False, True),
             "wave1": ("wave1", DTYPES[1:], False, False), "wave1_carry": ("wave1_carry", DTYPES[1:], True, False)}


def emu_step(emu, kind, prob, dtype, kernel, carry, linearize):
    code = P.KIND_CODE[kind]
    prm, u_max = P.params_of(kind, dtype).double().numpy(), P.u_max_of(kind)
    with np.errstate(all="ignore"):
        if kernel == "wave1_carry":
            import emu_row_carry
            rc, r = emu_row_carry.step(code, prm, P.DT, u_max, prob["x_init"], prob["C"], prob["c"], prob["F"], prob["cur_x"], prob["cur_u"],
                                       prob["lower"], prob["upper"], max_linesearch_iter=P.STEP_MAX_LS, linesearch_decay=P.STEP_DECAY)
            assert rc == 0, rc
            return r
        env = (code | (_native.ENV_CTRL_CARRY if carry else 0), prm, P.DT, u_max, linearize)
        F = np.zeros_like(prob["F"]) if linearize else prob["F"]
        return emu.lqr_step(prob["x_init"], prob["C"], prob["c"], F, None if linearize else prob["f"], prob["cur_x"], prob["cur_u"],
                            prob["lower"], prob["upper"], linesearch_decay=P.STEP_DECAY, max_linesearch_iter=P.STEP_MAX_LS, kernel=kernel,
                            dtype=NP[dtype], env=env)


def measure_steps(emu, kind):
    """{(stratum, dtype tag): c of the host build over the transitions of every emulated configuration}; env_points.check_step
    asserts its conditions on each run"""
    out = {}
    for config in sorted(EMU_STEPS):
        kernel, dtypes, carry, linearize = EMU_STEPS[config]
        for name in P.STEP_STRATA[kind]:
            for dtype in dtypes:
                tag = "f64" if dtype == torch.float64 else "f32"
                prob = P.step_problem(kind, name, dtype, carry)
                r = emu_step(emu, kind, prob, dtype, kernel, carry, linearize)
                c = P.check_step(kind, name, dtype, prob, r, carry, "%s %s %s %s" % (config, kind, name, tag))
                out[name, tag] = max(out.get((name, tag), 0.0), c)
    return out


@pytest.mark.parametrize("kind", P.KINDS)
def test_step_problems_on_the_emulated_bodies(emu_libs, kind):
    """The problems of tests/test_gpu_env_points.py's whole-step test through the emulator's builds of the same kernel bodies (tiny in both
    dtypes, with the carry, with in-kernel linearisation; wave1; wave1_carry): outputs finite, a problem that backtracks, a control on
    the box and one beyond u_max in every configuration, the cost of the returned trajectory -- and the host build's own c on the
    transitions these steps return, which env_points.C_HOST_STEP holds (see test_host_error_per_stratum for how the table is held to the measurement)."""
    for (name, tag), g in sorted(measure_steps(emu_libs, kind).items()):
        t = P.C_HOST_STEP[kind][name][tag]
        print("c_host step %-13s %-7s %s  %.2e (table %.1e)" % (kind, name, tag, g, t))
        eps = P.EPS[DTYPES[("f64", "f32").index(tag)]]
        assert g <= (max(4 * eps, t) if tag == "f64" else P.HOST_LIBM_MARGIN * t) and t <= max(2 * g, 4 * eps), (kind, name, tag, g, t)
