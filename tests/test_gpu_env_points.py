"""GPU tests (-m gpu) of the simulator transitions of csrc/env_dynamics.h on their device-only branches: the hardware sine /
cosine up to 32 rad and the library routines beyond, v_rcp_f32 / v_rsq_f32 with a Newton step, the clamp and its zero derivative,
the signed-zero atan2 of the full pendulum, the grid and wave tails of env_linearize_kernel (256 threads) and
env_traj_lane_kernel (64 lanes), the generic traj_cost_kernel, the control carry, and the simulator inside every step kernel.

Points, float64 reference, error unit and bounds: tests/env_points.py (its docstring; `bound`).  In short, with c_host the
error of the header's host build on the same stratum (env_points.C_HOST, measured by tests/test_env_points.py):
    float32, every trig argument within 32 rad:      |err| <= 2 c_host scale + 5e-6 (1 + |ref|)
    float32 beyond 32 rad, float64 everywhere:       |err| <= max(4 c_host, 4 eps) scale
Every comparison prints the device's own c (docs/history/r29.md has the table).

Measured on the MI355X: every case is inside its bound (worst err / bound 0.82 in float32, 0.70 in float64).  The first
run found four float64 cases of the full pendulum's f at 2.6 ... 7.5 times the 4-eps floor: an FMA in th + dt (w + dt acc) put
the angle one ulp off the reference's.  env_next_angle (csrc/env_dynamics.h) now takes the reference's roundings in float64;
the float32 kernels are byte for byte the parent's (docs/history/r29.md)."""
import functools

import numpy as np
import pytest
import torch

from mpc import _native
from oracle import env_oracle as E

import env_points as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float64, torch.float32)
IDS = ("f64", "f32")


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()            # fail loudly if the extension is missing
    return _native.HipBackend()


def env_of(kind, dtype):
    return P.dx_of(kind, dtype).native_env()


def linearize_nan(be, env, x, u):
    """mpc_env_linearize over NaN-filled outputs"""
    N, ns = x.shape
    F = torch.full((N, ns, ns + 1), float("nan"), dtype=x.dtype, device=x.device)
    f = torch.full((N, ns), float("nan"), dtype=x.dtype, device=x.device)
    be.env_linearize(env, x, u, out_F=F, out_f=f)
    torch.cuda.synchronize()
    return F, f


def successor(be, env, x, u):
    """the next state of every point: mpc_env_traj_cost with T = 2 (env_traj_lane_kernel)"""
    xs, _ = be.env_traj_cost(x, torch.stack((u, torch.zeros_like(u))), env)
    torch.cuda.synchronize()
    assert torch.equal(xs[0], x)
    return xs[1]


def device_outputs(be, kind, x, u):
    env = env_of(kind, x.dtype)
    xd, ud = x.to(DEV), u.to(DEV)
    F, f = linearize_nan(be, env, xd, ud)
    return {"next": successor(be, env, xd, ud), "F": F, "f": f}


# ---------------------------------------------------------------------------------------------
# (a) every kind, stratum and dtype
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", P.STRATA + ("edges",))
@pytest.mark.parametrize("kind", P.KINDS)
def test_linearize_and_transition_on_every_stratum(be, kind, name, dtype):
    """F and f from mpc_env_linearize, the next state from mpc_env_traj_cost with T = 2 on the same points.  The hand-made edge
    points are held to the fixture stratum's c_host; (0, 0) is compared on the transition only."""
    x, u = P.edges(kind, dtype) if name == "edges" else P.stratum(kind, name, dtype)
    got = device_outputs(be, kind, x, u)
    assert torch.isfinite(got["next"]).all()
    ch = {o: P.c_host(kind, "fixture" if name == "edges" else name, o, dtype) for o in P.OUTPUTS}
    P.compare(kind, dtype, x, u, got, ch, "device c %-13s %-7s %s" % (kind, name, IDS[DTYPES.index(dtype)]),
              no_jacobian=(P.EDGE_ORIGIN,) if name == "edges" else ())


# ---------------------------------------------------------------------------------------------
# (b) what must hold exactly
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", P.KINDS)
def test_linearize_exactness(be, kind, dtype):
    env, u_max = env_of(kind, dtype), P.u_max_of(kind)
    ex, eu = P.edges(kind, dtype)
    keep = [i for i in range(len(P.EDGE_NAMES)) if i != P.EDGE_ORIGIN]
    x = torch.cat([P.stratum(kind, s, dtype)[0] for s in P.STRATA] + [ex[keep]]).to(DEV)
    u = torch.cat([P.stratum(kind, s, dtype)[1] for s in P.STRATA] + [eu[keep]]).to(DEV)
    ns = x.shape[1]
    F, f = linearize_nan(be, env, x, u)
    F2, f2 = linearize_nan(be, env, x, u)
    assert torch.equal(F, F2) and torch.equal(f, f2), "two calls, same bits"
    assert torch.isfinite(F).all() and torch.isfinite(f).all(), "no NaN left of the pre-fill"
    outside = (u[:, 0].abs() > u_max)
    assert int(outside.sum()) > 6 * 0.15 * P.N
    assert (F[outside][:, :, ns] == 0).all(), "the clamp's derivative is zero outside the closed interval"
    for r, c in P.STRUCTURAL_ZEROS[kind]:
        assert (F[:, r, c] == 0).all(), (r, c)
    for r, c in P.STRUCTURAL_ONES[kind]:
        assert (F[:, r, c] == 1).all(), (r, c)
    if kind == "cartpole":
        assert (F[:, 0, 1] == torch.tensor(P.DT, dtype=dtype)).all()
    # the hand-made controls: the next number beyond +-u_max has a zero column; exactly on +-u_max the rows that do not depend on
    # the value of u carry the bits of an interior control at the same state
    Fe, _ = linearize_nan(be, env, ex.to(DEV), eu.to(DEV))
    assert (Fe[list(P.EDGE_BEYOND), :, ns] == 0).all()
    rows = P.U_FREE_ROWS[kind]
    inside = Fe[P.EDGE_INTERIOR][rows, ns]
    assert (inside != 0).all()
    for i in P.EDGE_ON_CLAMP:
        assert torch.equal(Fe[i][rows, ns], inside), P.EDGE_NAMES[i]
    if kind == "pendulum_full":
        a, b = P.EDGE_PI
        nxt = successor(be, env, ex.to(DEV), eu.to(DEV))
        ref = P.transition(kind, ex.double().numpy(), eu.double().numpy(), dtype)
        assert abs(ref[a, 2] - ref[b, 2]) > 0.09 and abs(float(nxt[a, 2] - nxt[b, 2])) > 0.09, "theta = +pi and -pi: dw differs by dt d 2 pi"


# ---------------------------------------------------------------------------------------------
# (c) tails and isolation
# ---------------------------------------------------------------------------------------------
LIN_SIZES = (1, 255, 256, 257, 513)
TRAJ_B = (1, 63, 64, 65, 130)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", P.KINDS)
def test_linearize_tails_and_isolation(be, kind, dtype):
    """N around the 256-thread block; the same bits as one larger call, which is itself held to the reference (the `past` points sit
    in its second and third block, where (a) never puts them); a NaN / inf point stays with itself; N = 0."""
    env = env_of(kind, dtype)
    x, u, ch = P.mixed(kind, ("fixture", "past"), P.N, dtype)            # 514 points
    xd, ud = x.to(DEV), u.to(DEV)
    F, f = linearize_nan(be, env, xd, ud)
    P.compare(kind, dtype, x, u, {"F": F, "f": f}, ch, "%s N = %d" % (kind, len(x)))
    for N in LIN_SIZES:
        Fn, fn = linearize_nan(be, env, xd[:N].contiguous(), ud[:N].contiguous())
        assert Fn.shape == (N,) + F.shape[1:] and torch.equal(Fn, F[:N]) and torch.equal(fn, f[:N]), N
    for bad in (float("nan"), float("inf")):
        for i in (0, 255, 256, 513):
            xb, ub = xd.clone(), ud.clone()
            xb[i], ub[i] = bad, bad
            Fb, fb = linearize_nan(be, env, xb, ub)
            others = torch.arange(len(x), device=DEV) != i
            assert torch.equal(Fb[others], F[others]) and torch.equal(fb[others], f[others]), (bad, i)
            assert not torch.isfinite(fb[i]).any() and not torch.isfinite(Fb[i]).all(), (bad, i)
    F0, f0 = be.env_linearize(env, xd[:0], ud[:0])
    assert F0.shape == (0,) + F.shape[1:] and f0.shape == (0, x.shape[1])


@functools.lru_cache(maxsize=None)
def _traj_inputs(kind, dtype, T):
    """B = 130.  T = 9: the fixture stratum under controls drawn from it; T <= 2: the fixture and past strata, 65 of each."""
    if T == 9:
        x, u0 = (t[:130] for t in P.stratum(kind, "fixture", dtype))
        g = torch.Generator().manual_seed(909)
        u = u0[torch.stack([torch.randperm(130, generator=g) for _ in range(T)]), 0].unsqueeze(2)
        return x, u.contiguous(), None
    x, u0, ch = P.mixed(kind, ("fixture", "past"), 65, dtype)
    return x, torch.stack([u0] * T), ch


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", P.KINDS)
def test_trajectory_tails_and_isolation(be, kind, dtype):
    """env_traj_lane_kernel at B around the 64-lane block and T = 1, 2, 9: all T states compared; the same bits as one larger call;
    a NaN / inf problem stays with itself; B = 0."""
    env = env_of(kind, dtype)
    tol = 1e-11 if dtype == torch.float64 else 5e-6
    for T in (1, 2, 9):
        x, u, ch = _traj_inputs(kind, dtype, T)
        xd, ud = x.to(DEV), u.to(DEV)
        full, cost = be.env_traj_cost(xd, ud, env)
        torch.cuda.synchronize()
        assert cost is None and full.shape == (T, 130, x.shape[1]) and torch.equal(full[0], xd)
        if T == 2:
            P.compare(kind, dtype, x, u[0], {"next": full[1]}, ch, "%s trajectory B = 130 T = 2" % kind)
        if T == 9:     # today's tolerance of tests/test_gpu_parity.py::test_env_kernels_match_reference_modules
            ref = E.traj(P.KIND_CODE[kind], x.double().numpy(), u.double().numpy(), P.params_of(kind, dtype).double().numpy())
            print(kind, "T = 9 max |x - ref|", float(np.abs(full.cpu().double().numpy() - ref).max()))
            np.testing.assert_allclose(full.cpu().double().numpy(), ref, rtol=tol * 20, atol=tol * 20)
        for B in TRAJ_B:
            part, _ = be.env_traj_cost(xd[:B].contiguous(), ud[:, :B].contiguous(), env)
            torch.cuda.synchronize()
            assert part.shape == (T, B, x.shape[1]) and torch.equal(part, full[:, :B]), (T, B)
        if T > 1:
            for bad in (float("nan"), float("inf")):
                for i in (0, 63, 64, 129):
                    xb, ub = xd.clone(), ud.clone()
                    xb[i], ub[:, i] = bad, bad
                    got, _ = be.env_traj_cost(xb, ub, env)
                    torch.cuda.synchronize()
                    others = torch.arange(130, device=DEV) != i
                    assert torch.equal(got[:, others], full[:, others]), (T, bad, i)
                    assert not torch.isfinite(got[:, i]).any(), (T, bad, i)
        empty, _ = be.env_traj_cost(xd[:0], ud[:, :0].contiguous(), env)
        assert empty.shape == (T, 0, x.shape[1])


# ---------------------------------------------------------------------------------------------
# (d) the other trajectory paths
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", P.KINDS)
def test_trajectory_with_cost_on_the_generic_kernel(be, kind, dtype):
    """C, c given: traj_cost_kernel (a workgroup per problem) runs the simulator.  The transition at the bounds of (a); the cost
    against env_oracle.quad_cost of the float64 trajectory: float64 rtol 1e-9, float32 1e-5 times the sum of |terms|."""
    env = env_of(kind, dtype)
    x, u, ch = _traj_inputs(kind, dtype, 2)
    T, B, n = 2, x.shape[0], x.shape[1] + 1
    g = torch.Generator().manual_seed(41)
    L = torch.randn(T, B, n, n, generator=g, dtype=torch.float64)
    C = (L @ L.transpose(2, 3) + 0.1 * torch.eye(n, dtype=torch.float64)).to(dtype)
    c = torch.randn(T, B, n, generator=g, dtype=torch.float64).to(dtype)
    xs, cost = be.env_traj_cost(x.to(DEV), u.to(DEV), env, C=C.to(DEV), c=c.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(xs[0], x.to(DEV))
    P.compare(kind, dtype, x, u[0], {"next": xs[1]}, ch, "%s traj_cost_kernel" % kind)
    ref_x = E.traj(P.KIND_CODE[kind], x.double().numpy(), u.double().numpy(), P.params_of(kind, dtype).double().numpy())
    Ch, ch_, uh = C.double().numpy(), c.double().numpy(), u.double().numpy()
    want = E.quad_cost(Ch, ch_, ref_x, uh)
    tau = np.concatenate((ref_x, uh), 2)
    terms = 0.5 * np.abs(tau[:, :, :, None] * Ch * tau[:, :, None, :]).sum((0, 2, 3)) + np.abs(ch_ * tau).sum((0, 2))
    err = np.abs(cost.cpu().double().numpy() - want)
    print(kind, dtype, "cost: max err / sum |terms| %.2e, max err / |cost| %.2e" % ((err / terms).max(), (err / np.abs(want)).max()))
    if dtype == torch.float64:
        np.testing.assert_allclose(cost.cpu().numpy(), want, rtol=1e-9)
    else:
        assert (err <= 1e-5 * terms).all(), (err / terms).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", P.KINDS)
def test_trajectory_behind_the_control_carry(be, kind, dtype):
    """EnvSpec.augmented(): the state is (u_prev, x).  The carried control comes back raw, bit for bit (beyond the clamp, too);
    the rest of every state is the simulator's successor of the kernel's own previous state, at the bounds of (a)."""
    env = env_of(kind, dtype).augmented()
    x, u0, ch = P.mixed(kind, ("fixture", "past"), 65, dtype)
    T, B = 3, x.shape[0]
    g = torch.Generator().manual_seed(43)
    u = torch.stack([u0[torch.randperm(B, generator=g)] for _ in range(T)]).contiguous()
    prev = torch.randn(B, 1, generator=g, dtype=torch.float64).to(dtype)
    z0 = torch.cat((prev, x), 1).to(DEV)
    zs, _ = be.env_traj_cost(z0, u.to(DEV), env)
    torch.cuda.synchronize()
    assert zs.shape == (T, B, x.shape[1] + 1) and torch.equal(zs[0], z0)
    assert torch.equal(zs[1:, :, 0], u.to(DEV)[:-1, :, 0]), "carried raw"
    assert float(u.abs().max()) > P.u_max_of(kind)
    for t in range(T - 1):
        P.compare(kind, dtype, zs[t, :, 1:].cpu(), u[t], {"next": zs[t + 1, :, 1:]}, ch, "%s carry t = %d" % (kind, t))


# ---------------------------------------------------------------------------------------------
# (e) the simulator inside every step kernel
# ---------------------------------------------------------------------------------------------
# configuration -> (impl, dtypes, control carry, in-kernel linearisation)
STEPS = {"generic": (_native.IMPL_GENERIC, DTYPES, False, False), "tiny": (_native.IMPL_TINY, DTYPES, False, False),
         "tiny_carry": (_native.IMPL_TINY, DTYPES, True, False), "tiny_linearize": (_native.IMPL_TINY, DTYPES, False, True),
         "wave1": (_native.IMPL_WAVE1, DTYPES[1:], False, False), "wave1_carry": (_native.IMPL_WAVE1_CARRY, DTYPES[1:], True, False)}


@pytest.mark.parametrize("config", sorted(STEPS))
@pytest.mark.parametrize("kind", P.KINDS)
def test_simulator_inside_the_step_kernels(be, kind, config):
    """One whole mpc_lqr_step (T = 5, B = 65) with the simulator as true dynamics, x_init from the fixture, fast and past strata
    (env_points.step_problem; tests/test_env_points.py runs the same problems through the emulated bodies).  Not compared with an
    oracle step: env_points.check_step asserts what isolates the transition from the sweep's rounding -- every returned
    new_x[t+1] against the float64 successor of the kernel's own (new_x[t], new_u[t]), the returned cost against the float64 cost
    of the returned trajectory -- and that some problem backtracked, some control ended on the box and some beyond u_max."""
    impl, dtypes, carry, linearize = STEPS[config]
    for name in P.STEP_STRATA[kind]:
        for dtype in dtypes:
            prob = P.step_problem(kind, name, dtype, carry)
            env = env_of(kind, dtype)
            if carry:
                env = env.augmented()
            env.linearize = linearize
            d = lambda k: torch.from_numpy(prob[k]).to(dtype).to(DEV)
            opts = _native.StepOptions(u_lower=prob["lower"], u_upper=prob["upper"], linesearch_decay=P.STEP_DECAY,
                                       max_linesearch_iter=P.STEP_MAX_LS, true_dynamics=env)
            r = be.lqr_step(d("x_init"), d("C"), d("c"), None if linearize else d("F"), None if linearize else d("f"), d("cur_x"),
                            d("cur_u"), opts, impl=impl)
            torch.cuda.synchronize()
            P.check_step(kind, name, dtype, prob, r, carry, "%s %s %s %s" % (config, kind, name, IDS[DTYPES.index(dtype)]))


# ---------------------------------------------------------------------------------------------
# (f) the range test itself
# ---------------------------------------------------------------------------------------------
def test_library_sine_and_cosine_beyond_32_rad(be):
    """In the unit of (a) a lost range test does not show: beyond 32 rad the hardware sine's own error, |x| 6e-8, is of the size
    of the float32 angle's rounding, eps A / 2, which that unit grants (docs/history/r29.md: a build with the threshold at 1e6
    passes `far`).  Here the argument is known exactly instead.  A cart-pole at (cos, sin) = (1, 0) returns (cos, sin)(dt w) as
    they come out of env_sincos, and dt w is ONE float32 product, the same on the host.  Against the float64 functions of that
    float32 number:
        |dt w| >  32 (library routines, 2 ulp of a value below 1, and 1 ulp of the normalisation):   |err| <= 4 eps
        |dt w| <= 32 (hardware, the header's 2e-6 at the threshold plus the instruction's own error): |err| <= 5e-6"""
    dtype, eps = torch.float32, P.EPS[torch.float32]
    env = env_of("cartpole", dtype)
    for name in ("fast", "edge32", "past", "far"):
        x, u = P.stratum("cartpole", name, dtype)
        x = x.clone()
        x[:, 2], x[:, 3] = 1.0, 0.0
        arg = (x[:, 4] * torch.tensor(P.DT, dtype=dtype)).double().numpy()
        nxt = successor(be, env, x.to(DEV), u.to(DEV)).cpu().double().numpy()
        err = np.maximum(np.abs(nxt[:, 2] - np.cos(arg)), np.abs(nxt[:, 3] - np.sin(arg)))
        beyond = np.abs(arg) > P.FAST_TRIG_MAX
        print("cart-pole at (1, 0), %-6s: %3d points beyond 32 rad, max |err| %.2e; %3d within, max |err| %.2e"
              % (name, beyond.sum(), err[beyond].max() if beyond.any() else 0.0, (~beyond).sum(), err[~beyond].max() if (~beyond).any() else 0.0))
        assert (err[beyond] <= 4 * eps).all() and (err[~beyond] <= P.DEVICE_BUDGET).all(), name
        if name == "edge32":
            assert beyond.sum() > 50 and (~beyond).sum() > 50
