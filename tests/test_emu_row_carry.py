"""CPU tests of the row-per-problem kernel's CARRY instantiation (csrc/lqr_wave1_body.h with -DMPC_WAVE1_CARRY, impl 10) through the
wavefront emulator (tests/emu_row_carry.py): one step against the lane-per-problem body (csrc/lqr_tiny_body.h compiled for the host,
the only other body that carries the control) on the same float32 inputs, and a row's independence of its three neighbours."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import emu_backend
import emu_row_carry as R
from conftest import ROOT
from mpc.dynamics import CtrlPassthroughDynamics
from mpc.env_dx import cartpole, pendulum
from oracle import lqr_oracle as O

CSRC = os.path.join(ROOT, "mpc.pytorch_amd", "csrc")
OUTPUTS = ("new_x", "new_u", "costs", "old_costs", "alphas", "full_du_norm", "alpha_du_norm", "K", "k")
TOL = dict({k: dict(rtol=1e-3, atol=1e-4) for k in OUTPUTS}, alphas=dict(rtol=1e-6, atol=0.0))     # tests/test_emu_unvouched.py, _WAVE1
TIE_CAP = 0.15                                  # tests/test_emu_mfma16.py, test_wavefront_per_problem_kernel
INDEFINITE = 8.0
T, B, BOUND = 9, 6, 0.4                          # a full wavefront and a half-empty one whose idle rows shadow the last problem

# the lane-per-problem body on the host, float32: every problem on one "lane" (the small source of tests/test_slew_planned.py's
# carry_step, for float instead of double and with every output)
HARNESS = r"""
#include "lqr_tiny_body.h"
using namespace mpclqr;

template <int NS>
static void step(int kind, const float *prm, float dt, float u_max, int T, int B, const float *x_init, const float *C, const float *c,
                 const float *F, const float *cur_x, const float *cur_u, float lo, float hi, int max_ls, float decay, float **out, float *ws)
{
    constexpr int N = NS + 1;
    StepParams<float> p = StepParams<float>();
    p.B = B; p.T = T; p.ns = NS; p.nc = 1;
    p.x_init = x_init; p.C = C; p.c = c; p.F = F; p.f = nullptr; p.cur_x = cur_x; p.cur_u = cur_u;
    p.C_st = (long)B * N * N; p.C_sb = N * N; p.c_st = (long)B * N; p.c_sb = N; p.F_st = (long)B * NS * N; p.F_sb = NS * N;
    p.bound_mode = MPC_BOUND_SCALAR; p.lo_s = lo; p.hi_s = hi;
    p.ls_decay = decay; p.max_ls = max_ls; p.pnqp_iter = 20;
    p.new_x = out[0]; p.new_u = out[1]; p.costs = out[2]; p.old_costs = out[3]; p.alphas = out[4]; p.full_du_norm = out[5];
    p.alpha_du_norm = out[6]; p.K = out[7]; p.k = out[8];
    p.env.kind = kind; p.env.linearize = F == nullptr; p.env.params = prm; p.env.dt = dt; p.env.u_max = u_max; p.env.carry = 1;
    float *Kw = ws, *Tw = ws + (long)T * N * B;
    for (int b = 0; b < B; ++b) tiny::lqr_step_problem<float, NS>(p, b, Kw, Tw, tiny::OneLane());
}
extern "C" void carry_step_f32(int kind, const float *prm, float dt, float u_max, int T, int B, const float *x_init, const float *C,
                               const float *c, const float *F, const float *cur_x, const float *cur_u, float lo, float hi, int max_ls,
                               float decay, float **out, float *ws)
{
    if (env_ns(kind) == 5) step<6>(kind, prm, dt, u_max, T, B, x_init, C, c, F, cur_x, cur_u, lo, hi, max_ls, decay, out, ws);
    else step<4>(kind, prm, dt, u_max, T, B, x_init, C, c, F, cur_x, cur_u, lo, hi, max_ls, decay, out, ws);
}
"""

# kind -> (the package's simulator, the reference's linesearch_decay for it (mpc/env_dx/pendulum.py:46, cartpole.py:60), the seed)
# (seeds at which the line search backtracks for some problem and no float32 body meets a tie of two trial costs)
SIMS = {"pendulum": (lambda: pendulum.PendulumDx(), 0.2, 6), "pendulum_full": (lambda: pendulum.PendulumDx(simple=False), 0.2, 6),
        "cartpole": (lambda: cartpole.CartpoleDx(), 0.5, 6)}


@pytest.fixture(scope="module")
def lane_lib(tmp_path_factory):
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    assert cxx, "needs clang++"
    d = tmp_path_factory.mktemp("row_carry")
    src, so = os.path.join(d, "harness.cpp"), os.path.join(d, "libharness.so")
    with open(src, "w") as fh:
        fh.write(HARNESS)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function",
                           "-I", CSRC, "-o", so, src])
    return ctypes.CDLL(so)


_CASES = {}


def case(kind):
    """The float32 inputs of one step around `kind`, made once: an augmented nominal z = (u_prev, x) that obeys the carried simulator
    (rolled out in float64 torch through CtrlPassthroughDynamics, then cast), a positive definite C, and the caller's augmented F for
    the runs without `linearize`, assembled from the PLAIN simulator's float32 Jacobian (host-compiled env_dynamics.h): carry row,
    zero column, the block inside."""
    if kind in _CASES:
        return _CASES[kind]
    make, decay, seed = SIMS[kind]
    dx = make()
    ns = dx.n_state
    NS, N = ns + 1, ns + 2
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    th = (torch.rand(B, generator=g, dtype=f64) - 0.5) * 2.5
    w = torch.randn(B, generator=g, dtype=f64)
    if ns == 3:
        x = torch.stack((th.cos(), th.sin(), w), 1)
    else:
        rr = 0.5 * torch.randn(B, 2, generator=g, dtype=f64)
        x = torch.stack((rr[:, 0], rr[:, 1], th.cos(), th.sin(), w), 1)
    u_prev = 0.3 * torch.randn(B, 1, generator=g, dtype=f64)
    z0 = torch.cat((u_prev, x), 1)
    cur_u = 0.3 * torch.randn(T, B, 1, generator=g, dtype=f64)
    dx64 = make()
    dx64.params = dx64.params.double()
    mod = CtrlPassthroughDynamics(dx64)
    zs = [z0]
    for t in range(T - 1):
        zs.append(mod(zs[-1], cur_u[t]))
    cur_x = torch.stack(zs)
    L = torch.randn(T, B, N, N, generator=g, dtype=f64)
    C = L @ L.transpose(2, 3) + 0.5 * torch.eye(N, dtype=f64)
    # (every other problem with an indefinite state block, as tests/test_emu_mfma16.py's "backtrack" case: the full step then raises the
    #  cost and the line search has to choose among its trials)
    C[:, 1::2, :NS, :NS] -= INDEFINITE * torch.eye(NS, dtype=f64)
    c = torch.randn(T, B, N, generator=g, dtype=f64)
    f32 = lambda t: np.ascontiguousarray(t.numpy(), np.float32)
    k = dict(kind=int(dx._kind), params=f32(dx.params), dt=float(dx.dt), u_max=float(dx._u_max), decay=decay, ns=ns, mod=mod,
             x_init=f32(z0), C=f32(C), c=f32(c), cur_x=f32(cur_x), cur_u=f32(cur_u))
    _, Je, _ = emu_backend.env_linearize(k["kind"], k["params"], k["dt"], k["u_max"], k["cur_x"][:-1].reshape(-1, NS)[:, 1:],
                                         k["cur_u"][:-1].reshape(-1), dtype=np.float32)
    F = np.zeros((T - 1, B, NS, N), np.float32)
    F[:, :, 0, N - 1] = 1.0
    F[:, :, 1:, 1:] = Je.reshape(T - 1, B, ns, ns + 1)
    k["F"] = F
    _CASES[kind] = k
    return k


def lane_step(lib, k, max_ls, linearize, **over):
    a = dict(k, **over)
    NS = k["ns"] + 1
    out = dict(new_x=np.full((T, B, NS), np.nan, np.float32), new_u=np.full((T, B, 1), np.nan, np.float32))
    for key in ("costs", "old_costs", "alphas", "full_du_norm", "alpha_du_norm"):
        out[key] = np.full(B, np.nan, np.float32)
    out["K"], out["k"] = np.full((T, B, 1, NS), np.nan, np.float32), np.full((T, B, 1), np.nan, np.float32)
    ptrs = (ctypes.c_void_p * 9)(*(out[key].ctypes.data for key in OUTPUTS[:2] + ("costs", "old_costs", "alphas", "full_du_norm",
                                                                                 "alpha_du_norm", "K", "k")))
    ws = np.zeros(2 * T * (NS + 1) * B, np.float32)
    vp, cf = ctypes.c_void_p, ctypes.c_float
    lib.carry_step_f32.argtypes = [ctypes.c_int, vp, cf, cf, ctypes.c_int, ctypes.c_int] + [vp] * 6 + [cf, cf, ctypes.c_int, cf, vp, vp]
    lib.carry_step_f32.restype = None
    lib.carry_step_f32(a["kind"], a["params"].ctypes.data, a["dt"], a["u_max"], T, B, a["x_init"].ctypes.data, a["C"].ctypes.data,
                       a["c"].ctypes.data, None if linearize else a["F"].ctypes.data, a["cur_x"].ctypes.data, a["cur_u"].ctypes.data,
                       -BOUND, BOUND, max_ls, a["decay"], ctypes.cast(ptrs, vp), ws.ctypes.data)
    return out


def row_step(k, max_ls, linearize, **over):
    a = dict(k, **over)
    rc, out = R.step(a["kind"], a["params"], a["dt"], a["u_max"], a["x_init"], a["C"], a["c"], None if linearize else a["F"], a["cur_x"],
                     a["cur_u"], -BOUND, BOUND, max_linesearch_iter=max_ls, linesearch_decay=a["decay"])
    assert rc == 0, rc
    return out


def oracle_alphas(k, max_ls):
    """The float64 step sizes: the oracle's sweep (oracle/lqr_oracle) on the augmented model -- its F from float64 autograd through
    CtrlPassthroughDynamics around the package's simulator at the nominal -- and the line search of mpc/lqr_step.py:176-247 with
    that module as the true dynamics."""
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    cur_x, cur_u, C, c, z0 = (f64(k[key]) for key in ("cur_x", "cur_u", "C", "c", "x_init"))
    NS = cur_x.shape[2]
    mod = k["mod"]
    zt = cur_x[:-1].reshape(-1, NS).clone().requires_grad_(True)
    ut = cur_u[:-1].reshape(-1, 1).clone().requires_grad_(True)
    nxt = mod(zt, ut)
    rows = [torch.cat(torch.autograd.grad(nxt[:, i].sum(), [zt, ut], retain_graph=True), 1) for i in range(NS)]
    F = torch.stack(rows, 1).reshape(T - 1, B, NS, NS + 1).numpy()
    # (F alone: the sweep of an iLQR step has no use for f, mpc/lqr_step.py:52-160 in delta space)
    o = O.lqr_step(z0.numpy(), C.numpy(), c.numpy(), F, None, cur_x.numpy(), cur_u.numpy(), -BOUND, BOUND, None, None, k["decay"], max_ls,
                   lockstep=False, return_gains=True)
    K, kk = f64(o["K"]), f64(o["k"])
    quad = lambda zz, uu, t: (0.5 * torch.einsum("bi,bij,bj->b", torch.cat((zz, uu), 1), C[t], torch.cat((zz, uu), 1))
                              + (torch.cat((zz, uu), 1) * c[t]).sum(1))
    old = sum(quad(cur_x[t], cur_u[t], t) for t in range(T))
    alphas, done = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.bool)
    alpha = 1.0
    with torch.no_grad():
        for j in range(max_ls):
            z, cost = z0, torch.zeros(B, dtype=torch.float64)
            for t in range(T):
                u = (torch.einsum("bij,bj->bi", K[t], z - cur_x[t]) + cur_u[t] + alpha * kk[t]).clamp(-BOUND, BOUND)
                cost = cost + quad(z, u, t)
                if t < T - 1:
                    z = mod(z, u)
            take = ~done & (~(cost > old) | (j == max_ls - 1))
            alphas[take] = alpha
            done |= take
            alpha *= k["decay"]
    return alphas.numpy()


@pytest.mark.parametrize("linearize", [True, False], ids=["linearize", "F_given"])
@pytest.mark.parametrize("max_ls", [1, 3, 10])
@pytest.mark.parametrize("kind", sorted(SIMS))
def test_emulated_carry_body_matches_the_lane_per_problem_body(lane_lib, kind, max_ls, linearize):
    """Every output at tests/test_emu_unvouched.py's _WAVE1 tolerances (1e-3 / 1e-4, alphas 1e-6).  A problem whose step size differs
    between the two float32 bodies is a float32 tie of two trial costs and is left out, at most 15 % of them
    (test_wavefront_per_problem_kernel's cap; at B = 6 that is none); the seeds are such that the lane body alone agrees with the
    float64 step sizes within the same cap, which is checked first."""
    k = case(kind)
    lane = lane_step(lane_lib, k, max_ls, linearize)
    ref = oracle_alphas(k, max_ls)
    assert (~np.isclose(lane["alphas"], ref, rtol=1e-6)).mean() <= TIE_CAP, (lane["alphas"], ref)
    assert max_ls == 1 or (ref < 1).any(), "some problem's line search must backtrack"
    row = row_step(k, max_ls, linearize)
    same = np.isclose(row["alphas"], lane["alphas"], rtol=1e-6)
    assert (~same).mean() <= TIE_CAP, (row["alphas"], lane["alphas"])
    for key in OUTPUTS:
        a, b = (v[same] if v.ndim == 1 else v[:, same] for v in (row[key], lane[key]))
        np.testing.assert_allclose(a, b, err_msg=key, **TOL[key])
    assert (np.abs(row["new_u"]) == np.float32(BOUND)).any() and (np.abs(row["new_u"]) < np.float32(BOUND)).any(), "some controls must clamp"
    # the carried control is the raw one, bit for bit
    assert np.array_equal(row["new_x"][1:, :, 0], row["new_u"][:-1, :, 0]) and np.array_equal(row["new_x"][0, :, 0], k["x_init"][:, 0])
    assert np.array_equal(row["new_x"][0], k["x_init"])


@pytest.mark.parametrize("poisoned", ["x_init", "c"])
@pytest.mark.parametrize("kind", ["pendulum", "cartpole"])
def test_a_row_does_not_depend_on_its_neighbours(kind, poisoned):
    """One of the four problems of wavefront 0 is given a NaN -- in x_init (its rollouts and costs are NaN) or in c (its sweep is, and the
    scalar QP's written-out form sends the whole wavefront through the loop: what pnqp1_fast's comment guards) --: the other three
    rows, and the second wavefront, answer bit for bit what they answer when that problem is finite."""
    k = case(kind)
    clean = row_step(k, 10, True)
    bad = np.array(k[poisoned], copy=True)
    if poisoned == "x_init":
        bad[1, 2] = np.nan
    else:
        bad[T // 2, 1, 1] = np.nan
    dirty = row_step(k, 10, True, **{poisoned: bad})
    assert not np.isfinite(dirty["costs"][1])
    others = [b for b in range(B) if b != 1]
    for key in OUTPUTS:
        a, b = (v[others] if v.ndim == 1 else v[:, others] for v in (dirty[key], clean[key]))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), key
    assert np.array_equal(dirty["status"][others], clean["status"][others]) and dirty["status"][1] & 2      # MPC_ST_NONFINITE


def test_the_carry_body_refuses_everything_but_a_carried_simulator():
    k = case("pendulum")
    args = (k["x_init"], k["C"], k["c"], None, k["cur_x"], k["cur_u"], -BOUND, BOUND)
    assert R.step(k["kind"], k["params"], k["dt"], k["u_max"], *args)[0] == 0
    assert R.step(k["kind"], k["params"], k["dt"], k["u_max"], *args, carry=False)[0] != 0                 # a plain simulator's flag at 4 states
    assert R.step(3, k["params"], k["dt"], k["u_max"], *args)[0] != 0                                      # the cart-pole at 4 states
    assert R.step(0, None, 0.0, 0.0, k["x_init"], k["C"], k["c"], k["F"], k["cur_x"], k["cur_u"], -BOUND, BOUND)[0] != 0     # a linear model
    assert R.step(k["kind"], k["params"], k["dt"], k["u_max"], *args, max_linesearch_iter=17)[0] != 0
