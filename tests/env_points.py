"""Shared by tests/test_env_points.py and tests/test_gpu_env_points.py: the points the simulator transitions of
mpc.pytorch_amd/csrc/env_dynamics.h are held to float64 on, their float64 reference, and the error unit.

Strata (N = 257 points each: one full 256-thread block of env_linearize plus one point; angles uniform on the circle; a
fifth of the controls outside the clamp, one exactly at +u_max and one at -u_max, as env_param_grad_ref.random_points):

    fixture   |w| <= 8            radius 0.75 ... 1.3      what the reference fixtures cover
    fast      40 <= |w| <= 600    radius 1                 __sinf / __cosf towards their limit (dt |w| up to 30 rad)
    edge32    dt |w| in [31.9, 32.1], half on each side    the range test |x| <= MPC_ENV_FAST_TRIG_MAX itself
    past      700 <= |w| <= 5000  radius 1                 the library branch
    far       4e4 <= |w| <= 1e5   radius 1                 |x / 2 pi| > 256: where v_sin_f32 is not defined
    radius    |w| <= 8            log-uniform 1e-3 ... 1e3 the Newton-refined v_rcp_f32 / v_rsq_f32, the normalisation

Reference: F and f from env_param_grad_ref.yardstick (float64 torch autograd through the package's own `_transition`,
which tests/test_host_logic.py ties to the reference's modules), the transition from oracle.env_oracle.step -- both at the
inputs and parameters as rounded to the dtype of the code under test.

Error unit.  A = 1 + the largest trig argument of the point (pendulum: dt (w + dt acc); full pendulum: max(|th + b|, |th2|);
cart-pole: dt |w|): rounding a float32 angle of magnitude A already costs eps A, so no fixed tolerance covers all strata.
    next state, F:   scale = (1 + |ref|) A
    f = next - F tau: scale = (|next| + sum_j |F_rj| |tau_j|) A      (the cancellation scale)
    c = max over entries and points of |got - ref| / scale

C_HOST is c of the HOST build of env_dynamics.h (tests/emu_backend.env_linearize: libm and IEEE division), what the number
format can do on these points -- not a measurement of the device path.  tests/test_env_points.py measures it again on every
run and holds this table to the measurement; tests/test_gpu_env_points.py takes its bounds from the table, so that the GPU
suite needs no emulator build."""
import functools

import numpy as np
import torch

import env_param_grad_ref as R
from oracle import env_oracle as E

KINDS = R.KINDS
KIND_CODE = {"pendulum": E.PENDULUM, "pendulum_full": E.PENDULUM_FULL, "cartpole": E.CARTPOLE}
STRATA = ("fixture", "fast", "edge32", "past", "far", "radius")
OUTPUTS = ("next", "F", "f")
N = 257
FAST_TRIG_MAX = 32.0            # MPC_ENV_FAST_TRIG_MAX
EDGE_BAND = 1e-4                # a trig argument this close to the threshold may take either branch (see `bound`)
HOST_LIBM_MARGIN = 1.3         # tests/test_env_points.py only: a float32 figure measured on another host may exceed the table by this
DEVICE_BUDGET = 5e-6            # what tests/test_gpu_parity.py grants the device substitutions on the fixtures (rtol = atol)
EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}
DT = E.DT
_SEED = {s: 2900 + 10 * i for i, s in enumerate(STRATA)}


def dx_of(kind, dtype=torch.float64):
    return R.make_dx(kind, torch.tensor(R.PARAMS[kind], dtype=dtype))


def u_max_of(kind):
    return float(dx_of(kind)._u_max)


def _signed(g, lo, hi, n):
    mag = lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)
    return mag * (2.0 * (torch.rand(n, generator=g, dtype=torch.float64) < 0.5) - 1.0)


@functools.lru_cache(maxsize=None)
def _stratum64(kind, stratum):
    g = torch.Generator().manual_seed(_SEED[stratum] + KINDS.index(kind))
    f64 = torch.float64
    u_max = u_max_of(kind)
    th = (torch.rand(N, generator=g, dtype=f64) - 0.5) * 2 * (np.pi - 2e-3)       # (2e-3 rad kept clear of atan2's branch cut)
    r = torch.ones(N, dtype=f64)
    if stratum in ("fixture", "radius"):
        w = (torch.rand(N, generator=g, dtype=f64) - 0.5) * 16.0
        u01 = torch.rand(N, generator=g, dtype=f64)
        r = 0.75 + 0.55 * u01 if stratum == "fixture" else 10.0 ** (6.0 * u01 - 3.0)
    elif stratum == "fast":
        w = _signed(g, 40.0, 600.0, N)
    elif stratum == "edge32":
        w = _signed(g, 31.9 / DT, 32.0 / DT, N)
        w[1::2] = _signed(g, 32.0 / DT, 32.1 / DT, N)[1::2]
    elif stratum == "past":
        w = _signed(g, 700.0, 5000.0, N)
    else:
        w = _signed(g, 4e4, 1e5, N)
    c, s = r * th.cos(), r * th.sin()
    if kind == "cartpole":
        z = torch.randn(N, 2, generator=g, dtype=f64)
        x = torch.stack((z[:, 0], z[:, 1], c, s, w), 1)
    else:
        x = torch.stack((c, s, w), 1)
    u = (torch.rand(N, 1, generator=g, dtype=f64) - 0.5) * 2.5 * u_max
    u[N // 3, 0], u[(2 * N) // 3, 0] = u_max, -u_max
    return x, u


def stratum(kind, name, dtype=torch.float64):
    """(x [N, ns], u [N, 1]) of one stratum, rounded to `dtype`"""
    x, u = _stratum64(kind, name)
    return x.to(dtype), u.to(dtype)


EDGE_NAMES = ("theta=+pi", "theta=-pi", "origin", "+u_max", "-u_max", "beyond +u_max", "beyond -u_max", "interior")
EDGE_ORIGIN, EDGE_PI = 2, (0, 1)
EDGE_ON_CLAMP, EDGE_BEYOND, EDGE_INTERIOR = (3, 4), (5, 6), 7
# rows of the control column of F that do not depend on the value of u (only on the clamp's derivative), and the entries of F
# that are zero by structure (env_dynamics.h: the cart-pole's `for (i < 30) J[i] = 0` and what it then leaves; the pendulums' J[10] = 1
# is their only constant, the simple pendulum's w_c its only zero)
U_FREE_ROWS = {"pendulum": [2], "pendulum_full": [2], "cartpole": [1, 4]}
STRUCTURAL_ZEROS = {"pendulum": [(2, 0)], "pendulum_full": [],
                    "cartpole": [(0, 2), (0, 3), (0, 4), (0, 5), (1, 0), (2, 0), (2, 1), (2, 5), (3, 0), (3, 1), (3, 5), (4, 0), (4, 1)]}
STRUCTURAL_ONES = {"pendulum": [(2, 2)], "pendulum_full": [(2, 2)], "cartpole": [(0, 0), (1, 1)]}


def edges(kind, dtype=torch.float64):
    """The hand-made points, EDGE_NAMES in order: (cos, sin) = (-1, +0.0), (-1, -0.0) and (0, 0) at an interior control; then
    one ordinary state at u = +-u_max exactly, at the next number of `dtype` beyond each, and at an interior control."""
    u_max = u_max_of(kind)
    cs = [(-1.0, 0.0), (-1.0, -0.0), (0.0, 0.0)] + [(np.cos(0.9), np.sin(0.9))] * 5
    one = torch.tensor(u_max, dtype=dtype)
    up = float(torch.nextafter(one, torch.tensor(np.inf, dtype=dtype)))
    us = [0.3 * u_max] * 3 + [u_max, -u_max, up, -up, 0.3 * u_max]
    rows = [((0.4, -0.3) if kind == "cartpole" else ()) + (c, s, 0.7) for c, s in cs]
    x = torch.tensor(rows, dtype=torch.float64).to(dtype)
    u = torch.tensor(us, dtype=torch.float64).reshape(-1, 1).to(dtype)
    assert float(u[5, 0]) > u_max and float(u[6, 0]) < -u_max and float(u[3, 0]) == u_max
    return x, u


def params_of(kind, dtype):
    """the parameters as the code under test holds them: rounded to its dtype"""
    return torch.tensor(R.PARAMS[kind], dtype=dtype)


def transition(kind, x, u, dtype):
    """float64 oracle.env_oracle.step at x [N, ns], u [N, 1] (tensors or arrays, taken as they are)"""
    prm = params_of(kind, dtype).double().numpy()
    return E.step(KIND_CODE[kind], np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64), prm)


def reference(kind, x, u, dtype=None):
    """float64 (next, F, f, A) as numpy arrays at the points x, u (already rounded to `dtype`, default: their own)"""
    dtype = x.dtype if dtype is None else dtype
    x, u = x.detach().cpu().double(), u.detach().cpu().double()
    n, ns = x.shape
    F, f, _, _ = R.yardstick(kind, params_of(kind, dtype), x, u, torch.zeros(n, ns, ns + 1, dtype=torch.float64),
                             torch.zeros(n, ns, dtype=torch.float64))
    with np.errstate(all="ignore"):
        nxt = transition(kind, x.numpy(), u.numpy(), dtype)
    return nxt, F.numpy(), f.numpy(), trig_unit(kind, x.numpy(), nxt, dtype)


def trig_unit(kind, x, nxt, dtype):
    """A = 1 + the largest trig argument of every point (x the state, nxt its float64 successor)"""
    if kind == "cartpole":
        arg = DT * np.abs(x[:, 4])
    elif kind == "pendulum":
        arg = np.abs(DT * nxt[:, 2])
    else:
        th = np.arctan2(x[:, 1], x[:, 0])
        b = float(params_of(kind, dtype)[4])
        arg = np.maximum(np.abs(th + b), np.abs(th + DT * nxt[:, 2]))
    return 1.0 + arg


def scales(x, u, nxt, F, A):
    """{output: scale}, shaped like the outputs"""
    tau = np.concatenate((np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)), 1)
    cancel = np.abs(nxt) + (np.abs(F) * np.abs(tau)[:, None, :]).sum(2)
    return {"next": (1 + np.abs(nxt)) * A[:, None], "F": (1 + np.abs(F)) * A[:, None, None], "f": cancel * A[:, None]}


def c_of(got, ref, scale, keep=None):
    """max |got - ref| / scale over the points `keep` (default: all)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if keep is not None:
        got, ref, scale = got[keep], ref[keep], scale[keep]
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        q = np.abs(got - ref) / scale
    return float(np.max(np.where(np.isnan(q), np.inf, q)))


def bound(output, dtype, c_host, ref, scale, A):
    """The device's error bound, shaped like `ref`.
      float32, every trig argument of the point within 32 rad (the hardware's sine / cosine, reciprocal and rsqrt):
          2 c_host scale + 5e-6 (1 + |ref|); for f the second term is 5e-6 times the cancellation scale without A
      float32 beyond 32 rad, float64 everywhere (library routines):   max(4 c_host, 4 eps) scale
    The kernel forms its argument in float32, a few eps A ~ 1e-5 off the float64 one that A is made of: a point whose
    argument lies within EDGE_BAND of the threshold may have taken either branch and gets the larger of the two."""
    per_point = (-1,) + (1,) * (ref.ndim - 1)
    c_host = np.asarray(c_host, dtype=np.float64)          # one figure, or one per point (points of several strata in one call)
    if c_host.ndim:
        c_host = c_host.reshape(per_point)
    lib = np.maximum(4.0 * c_host, 4.0 * EPS[dtype]) * scale
    if dtype == torch.float64:
        return lib
    a = A.reshape(per_point)
    unit = scale / a if output == "f" else 1 + np.abs(ref)
    fast = 2.0 * c_host * scale + DEVICE_BUDGET * unit
    arg = a - 1.0
    return np.where(arg <= FAST_TRIG_MAX - EDGE_BAND, fast, np.where(arg > FAST_TRIG_MAX + EDGE_BAND, lib, np.maximum(fast, lib)))


# c of the host build, [kind][stratum][dtype name] -> (next, F, f): the figures tests/test_env_points.py measures (its docstring
# has the table), rounded UP in the last digit printed and nothing more, so that the device's bounds are the issue's 2 c_host and
# 4 c_host.  That test fails when a figure here is more than twice what it measures; the room it leaves another host's libm
# (HOST_LIBM_MARGIN) is applied there, on the CPU, and never in `bound`.
C_HOST = {
    "pendulum": {
        "fixture": {"f64": (2.1e-16, 2.2e-16, 2.0e-15), "f32": (7.3e-08, 1.2e-07, 1.5e-07)},
        "fast": {"f64": (1.2e-16, 1.1e-16, 8.2e-16), "f32": (8.4e-08, 7.6e-08, 7.9e-07)},
        "edge32": {"f64": (1.1e-16, 9.0e-17, 2.5e-15), "f32": (8.7e-08, 7.9e-08, 1.1e-06)},
        "past": {"f64": (7.7e-17, 7.5e-17, 4.1e-15), "f32": (8.1e-08, 8.3e-08, 6.3e-06)},
        "far": {"f64": (9.2e-17, 8.7e-17, 1.1e-14), "f32": (8.3e-08, 7.8e-08, 1.1e-05)},
        "radius": {"f64": (7.3e-16, 3.6e-15, 1.4e-15), "f32": (2.3e-07, 6.0e-07, 1.6e-06)},
    },
    "pendulum_full": {
        "fixture": {"f64": (7.4e-17, 9.6e-17, 1.2e-16), "f32": (5.1e-08, 7.1e-08, 2.4e-07)},
        "fast": {"f64": (0.0e+00, 2.9e-17, 3.6e-17), "f32": (9.5e-08, 8.4e-08, 1.1e-06)},
        "edge32": {"f64": (0.0e+00, 4.3e-18, 5.8e-18), "f32": (1.2e-07, 9.2e-08, 3.1e-06)},
        "past": {"f64": (0.0e+00, 2.1e-18, 2.7e-18), "f32": (1.2e-07, 9.8e-08, 3.8e-06)},
        "far": {"f64": (0.0e+00, 3.8e-20, 0.0e+00), "f32": (9.4e-08, 9.2e-08, 7.1e-06)},
        "radius": {"f64": (5.3e-17, 2.5e-16, 9.5e-17), "f32": (6.0e-08, 4.1e-06, 1.3e-07)},
    },
    "cartpole": {
        "fixture": {"f64": (6.0e-16, 2.7e-16, 1.5e-15), "f32": (5.1e-07, 1.4e-07, 1.5e-07)},
        "fast": {"f64": (2.8e-15, 2.0e-16, 1.6e-15), "f32": (3.4e-07, 5.7e-08, 6.9e-07)},
        "edge32": {"f64": (2.4e-16, 9.0e-17, 1.3e-15), "f32": (2.5e-07, 5.7e-08, 1.5e-06)},
        "past": {"f64": (9.9e-17, 9.9e-17, 9.1e-15), "f32": (6.4e-08, 5.2e-08, 2.3e-06)},
        "far": {"f64": (9.8e-17, 8.5e-17, 9.0e-14), "f32": (6.8e-08, 6.3e-08, 6.9e-05)},
        "radius": {"f64": (1.1e-14, 1.1e-14, 2.1e-14), "f32": (2.9e-05, 5.9e-05, 5.8e-05)},
    },
}


def c_host(kind, name, output, dtype):
    return C_HOST[kind][name]["f64" if dtype == torch.float64 else "f32"][OUTPUTS.index(output)]


def mixed(kind, names, per, dtype):
    """The first `per` points of each of the strata `names`, one after the other: (x, u, {output: c_host of every point})"""
    xs, us = zip(*(tuple(t[:per] for t in stratum(kind, s, dtype)) for s in names))
    ch = {o: np.concatenate([np.full(per, c_host(kind, s, o, dtype)) for s in names]) for o in OUTPUTS}
    return torch.cat(xs), torch.cat(us), ch


def compare(kind, dtype, x, u, got, ch, what, no_jacobian=()):
    """Hold the outputs got = {output: [N, ...]} at the points x [N, ns], u [N, 1] (as the kernel got them, `dtype`) to `bound`
    with c_host = ch[output] (a figure or one per point); the points `no_jacobian` are compared on the transition only.
    Prints and returns the code's own c per output."""
    nxt, F, f, A = reference(kind, x, u, dtype)
    xh, uh = x.detach().cpu().double().numpy(), u.detach().cpu().double().numpy()
    sc, ref, out, fails = scales(xh, uh, nxt, F, A), dict(zip(OUTPUTS, (nxt, F, f))), {}, []
    for o, g in got.items():
        g = (g.detach().cpu() if torch.is_tensor(g) else torch.as_tensor(g)).double().numpy()
        keep = np.ones(len(g), bool)
        if o != "next":
            keep[list(no_jacobian)] = False
        assert g.shape == ref[o].shape and np.isfinite(ref[o][keep]).all(), (what, o)
        b = bound(o, dtype, ch[o], ref[o], sc[o], A)
        with np.errstate(invalid="ignore"):
            ratio = np.where(keep.reshape((-1,) + (1,) * (g.ndim - 1)), np.abs(g - ref[o]) / b, 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        out[o] = c_of(g, ref[o], sc[o], keep)
        n_bad = int((ratio > 1).sum())
        print("%s %-4s c = %.2e  worst err / bound %.2f" % (what, o, out[o], ratio.max()))
        if n_bad:
            i = int(np.argmax(ratio.reshape(len(g), -1).max(1)))
            fails.append("%s %s: %d entries beyond the bound, worst err / bound %.3g at point %d (A = %.4g)" % (what, o, n_bad, ratio.max(), i, A[i]))
    assert not fails, fails
    return out


# ---------------------------------------------------------------------------------------------
# One whole LQR step with the simulator as true dynamics: the problem, and what isolates the transition inside the step
# kernels from the sweep's own rounding
# ---------------------------------------------------------------------------------------------
STEP_T, STEP_B = 5, 65
# (no `past` for the cart-pole: its Jacobian reaches 1e5 there)
STEP_STRATA = {"pendulum": ("fixture", "fast", "past"), "pendulum_full": ("fixture", "fast", "past"), "cartpole": ("fixture", "fast")}
STEP_R = {"pendulum": 0.05, "pendulum_full": 0.05, "cartpole": 1e-3}          # the control's weight
STEP_DECAY, STEP_MAX_LS = 0.2, 10


def step_problem(kind, name, dtype, carry=False):
    """float64 arrays, every value rounded to `dtype`: x_init = the first STEP_B states of the stratum, a nominal rolled out
    through the float64 simulator, F and f from the float64 reference at the nominal, the box +-1.5 u_max (so that rolled-out
    controls pass the simulator's own clamp).
    Every fourth problem is PUSHED: its nominal control sits at 0.99 u_max and a linear cost on the velocity that answers the
    control asks for more of it.  The linear model promises a gain all the way to the box; the simulator clamps at u_max and
    returns only the control's own cost, so the full step is worse than the nominal and the line search backtracks.
    carry: the problem behind the control carry, z = (u_prev, x), with a slew term STEP_R (u - u_prev)^2 / 2 in the cost."""
    T, B = STEP_T, STEP_B
    rd = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype).double().numpy()
    code, u_max, prm = KIND_CODE[kind], u_max_of(kind), params_of(kind, dtype).double().numpy()
    g = np.random.RandomState(290 + STRATA.index(name))
    x0 = stratum(kind, name, dtype)[0][:B].double().numpy()
    ns = x0.shape[1]
    n = ns + 1
    cur_u = 0.9 * u_max * (2 * g.rand(T, B, 1) - 1)
    push = np.arange(0, B, 4)
    sgn = np.where(np.arange(len(push)) % 2 == 0, 1.0, -1.0)            # alternately towards +u_max and -u_max
    cur_u[:, push, 0] = 0.99 * u_max * sgn
    cur_u = rd(cur_u)
    cur_x = rd(E.traj(code, x0, cur_u, prm))
    lin = [reference(kind, torch.from_numpy(cur_x[t]), torch.from_numpy(cur_u[t]), dtype) for t in range(T - 1)]
    F, f = rd(np.stack([l[1] for l in lin])), rd(np.stack([l[2] for l in lin]))
    q = np.ones(n)
    q[ns - 1], q[ns] = 0.0, STEP_R[kind]                                # (no weight of its own on the angular velocity: 5000^2 at `past`)
    if kind == "cartpole":
        q[0] = q[1] = 0.1
    L = 0.1 * g.randn(T, B, n, n)
    C = np.einsum("tbik,tbjk->tbij", L, L) * np.sqrt(q)[:, None] * np.sqrt(q)[None, :] + np.diag(q)
    c = g.randn(T, B, n) * np.sqrt(q)
    c[:, :, ns] = 2.0 * STEP_R[kind] * u_max * g.randn(T, B)
    row = 1 if kind == "cartpole" else ns - 1           # the velocity that answers the control with a sign that does not change
    Fu = F[:, push, row, ns]
    c[:, push, :] = 0.0
    c[1:, push, row] = -sgn * np.sign(Fu) * 3.0 * STEP_R[kind] * u_max / np.abs(Fu)
    out = dict(x_init=x0, C=rd(C), c=rd(c), F=F, f=f, cur_x=cur_x, cur_u=cur_u, lower=-1.5 * u_max, upper=1.5 * u_max, pushed=push)
    if carry:
        prev = rd(u_max * (2 * g.rand(B, 1) - 1))
        gamma = STEP_R[kind]
        aC = np.zeros((T, B, n + 1, n + 1))
        aC[:, :, 1:, 1:] = out["C"]
        aC[:, :, 0, 0] += gamma; aC[:, :, n, n] += gamma; aC[:, :, 0, n] -= gamma; aC[:, :, n, 0] -= gamma
        ac = np.zeros((T, B, n + 1))
        ac[:, :, 1:] = out["c"]
        aF = np.zeros((T - 1, B, ns + 1, n + 1))         # the carry row (0 ... 0 1), a zero column for u_prev, the simulator's block
        aF[:, :, 0, n], aF[:, :, 1:, 1:] = 1.0, F
        af = np.zeros((T - 1, B, ns + 1))
        af[:, :, 1:] = f
        z = np.concatenate((np.concatenate((prev[None], cur_u[:-1])), cur_x), 2)
        out.update(x_init=z[0].copy(), C=rd(aC), c=ac, F=aF, f=af, cur_x=z)
    return out


# c (next state) of the HOST build on the points the emulated step kernels return for these problems, the largest over the
# emulated configurations; the measured figures rounded up in the last digit, held to the measurement like C_HOST
C_HOST_STEP = {
    "pendulum": {"fixture": {"f64": 2.9e-16, "f32": 8.0e-08}, "fast": {"f64": 1.3e-16, "f32": 8.1e-08}, "past": {"f64": 1.9e-16, "f32": 7.7e-08}},
    "pendulum_full": {"fixture": {"f64": 8.9e-17, "f32": 3.8e-08}, "fast": {"f64": 8.5e-17, "f32": 1.2e-07}, "past": {"f64": 0.0e+00, "f32": 1.3e-07}},
    "cartpole": {"fixture": {"f64": 6.0e-16, "f32": 3.2e-07}, "fast": {"f64": 2.0e-15, "f32": 2.2e-06}},
}


def _host(a):
    return (a.detach().cpu() if torch.is_tensor(a) else torch.as_tensor(a)).double().numpy()


def check_step(kind, name, dtype, prob, r, carry, what):
    """r: the step's outputs (new_x, new_u, costs, alphas; tensors or arrays).  Asserted:
      - every output finite, new_x[0] = x_init bit for bit, a carried control raw and bit for bit;
      - for every t and problem, new_x[t+1] is the float64 successor of the kernel's own (new_x[t], new_u[t]) within the bound of
        one transition (`bound`) with c_host = C_HOST_STEP: the host build's error on the points these steps visit.  (They are
        not the stratum's points: other controls -- on the box, far beyond the clamp -- and, from t = 1 on, other states.  The
        cart-pole's w + dt * th_acc cancels from 550 to 0.6 at one of them, where the host build itself has c = 1.6e-6
        against the `fast` stratum's 3.4e-7.);
      - costs = the float64 cost of the returned trajectory, within 1e-5 (float32) / 1e-11 (float64) times the sum of |terms|;
      - the conditions that make the run worth having: a problem that backtracked, a control on the box, a control beyond u_max."""
    new_x, new_u, costs, alphas = (_host(r[k]) for k in ("new_x", "new_u", "costs", "alphas"))
    T, B = new_u.shape[:2]
    u_max = u_max_of(kind)
    assert all(np.isfinite(a).all() for a in (new_x, new_u, costs, alphas)), what
    assert np.array_equal(new_x[0], prob["x_init"]), what
    sim = new_x[:, :, 1:] if carry else new_x
    if carry:
        assert np.array_equal(new_x[1:, :, 0], new_u[:-1, :, 0]), "carried raw"
    ch = {"next": C_HOST_STEP[kind][name]["f64" if dtype == torch.float64 else "f32"]}
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)      # (exact: these are the kernel's own numbers)
    c_next = max(compare(kind, dtype, to(sim[t]), to(new_u[t]), {"next": sim[t + 1]}, ch, "%s t = %d" % (what, t))["next"] for t in range(T - 1))
    # for the reader: would the stratum's own c_host have held as well?  (not asserted: it does not on the cart-pole's `fast`)
    worst = 0.0
    for t in range(T - 1):
        nxt, F, _, A = reference(kind, to(sim[t]), to(new_u[t]), dtype)
        sc = scales(sim[t], new_u[t], nxt, F, A)["next"]
        worst = max(worst, float((np.abs(sim[t + 1] - nxt) / bound("next", dtype, c_host(kind, name, "next", dtype), nxt, sc, A)).max()))
    print("%s with the stratum's c_host %.1e instead of %.1e: worst err / bound %.2f (%s)"
          % (what, c_host(kind, name, "next", dtype), ch["next"], worst, "would hold" if worst <= 1 else "would NOT hold"))
    tau = np.concatenate((new_x, new_u), 2)
    want = E.quad_cost(prob["C"], prob["c"], new_x, new_u)
    terms = 0.5 * np.abs(tau[:, :, :, None] * prob["C"] * tau[:, :, None, :]).sum((0, 2, 3)) + np.abs(prob["c"] * tau).sum((0, 2))
    err = np.abs(costs - want) / terms
    print("%s cost: max err / sum |terms| %.2e" % (what, err.max()))
    assert (err <= (1e-11 if dtype == torch.float64 else 1e-5)).all(), (what, err.max())
    n_back, n_box, n_beyond = int((alphas < 1).sum()), int((np.abs(new_u) == 1.5 * u_max).sum()), int((np.abs(new_u) > u_max).sum())
    print("%s backtracked %d, controls on the box %d, beyond u_max %d" % (what, n_back, n_box, n_beyond))
    assert n_back > 0 and n_box > 0 and n_beyond > 0, (what, n_back, n_box, n_beyond)
    return c_next
