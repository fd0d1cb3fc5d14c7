"""On the device: HipBackend.lqr_step, impl 0 and every forced impl that takes the shape, on the two matrices of
tests/test_emu_unvouched.py -- a bare call whose nominal is off x_init (the reference: dx_0 = 0, new_x[0] = x_init,
mpc/lqr_step.py:181-182), and batches with non-finite problems -- plus the other ways a step reaches the device: the sweep / rollout
pair, the network rollout, a shipped simulator as true_dynamics, and the LQRStep module.

Tolerances are the device tests' own.  float32: rtol 1e-3 / atol 1e-4 on trajectories and gains, rtol 2e-4 on costs, rtol 1e-5 on
old_costs, rtol 1e-3 / atol 1e-4 on the du norms (tests/test_gpu_narrow.py, test_padded_mfma40_shapes_between_the_tuned_ones);
float64: rtol 1e-9 / atol 1e-10 (test_degenerate_sizes_every_kernel).  A problem whose line search lands on another alpha than the
oracle's may be left out of the trajectory comparison, at most one per case (the same tests' cap); the seeds are those for which
the oracle's own float32 and float64 runs agree on every alpha (tests/unvouched_gpu_seeds.py, checked on the CPU by
tests/test_emu_unvouched.py), so the cap is never what hides a shifted problem."""
import numpy as np
import pytest
import torch

import unvouched_cases as U
import unvouched_gpu_seeds as S
from conftest import golden
from mpc import _native
from mpc._native import StepOptions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ST_NONFINITE, ST_OFF, ST_ASYM = 2, 4, 8
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()
    return _native.HipBackend()


def host(t):
    return t.detach().cpu().numpy()


def dev(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


# (impl, dtype, n_state, n_ctrl, B, the emulator test's kernel family, which kernel verifies the nominal)
# impl 1 at the shapes tests/test_gpu_generic.py routes there; impl 0 at one shape per kernel it picks.
ROWS = [
    (0, F32, 12, 4, 9, "dpp", "dpp16"), (0, F32, 10, 3, 9, "dpp", "dpp16"), (0, F32, 32, 8, 3, "m40", "mfma40"),
    (0, F32, 13, 4, 3, "pad", "mfma40"), (0, F32, 16, 4, 3, "pad", "mfma40"), (0, F32, 3, 1, 70, "tiny_f32", "none"),
    (0, F64, 12, 4, 3, "m16_f64", "none"), (0, F64, 3, 1, 70, "tiny_f64", "none"),
    (1, F64, 21, 4, 3, "generic", "none"), (1, F32, 33, 2, 3, "generic", "none"), (1, F64, 12, 4, 3, "generic", "none"),
    (2, F32, 12, 4, 3, "m16", "none"), (2, F32, 5, 2, 3, "m16", "none"), (2, F64, 12, 4, 3, "m16_f64", "none"), (2, F64, 5, 2, 3, "m16_f64", "none"),
    (3, F32, 12, 4, 9, "dpp", "dpp16"), (8, F32, 10, 3, 9, "dpp", "dpp16"), (8, F32, 12, 4, 9, "dpp", "dpp16"),
    (4, F32, 3, 1, 70, "tiny_f32", "none"), (4, F64, 3, 1, 70, "tiny_f64", "none"), (6, F32, 3, 1, 9, "wave1", "none"),
    (5, F32, 32, 8, 3, "m40", "mfma40"), (7, F32, 13, 4, 3, "pad", "mfma40"), (7, F32, 16, 4, 3, "pad", "mfma40"),
    (9, F32, 13, 4, 3, "pad", "mfma40"), (9, F32, 16, 4, 3, "pad", "mfma40"),
]
ROW_IDS = ["impl%d-%s-%d_%d" % (r[0], "f32" if r[1] == F32 else "f64", r[2], r[3]) for r in ROWS]
CASES = [(m, 6, True) for m in U.MODES] + [("free", 6, False), ("box", 6, False), ("free", 1, True)]


def options(kw, dt, **more):
    lo, hi = kw.get("u_lower"), kw.get("u_upper")
    if isinstance(lo, np.ndarray):
        lo, hi = dev(lo, dt), dev(hi, dt)
    zm = kw.get("u_zero_I")
    return StepOptions(u_lower=lo, u_upper=hi, delta_u=kw.get("delta_u"), u_zero_I=None if zm is None else torch.from_numpy(zm).to(DEV), **more)


def run_step(be, kw, dt, impl, vouch=False):
    """One mpc_lqr_step through a bound plan whose trajectory buffers are pre-filled with NaN (an element the kernel leaves
    unwritten shows), and the gains from a second, unplanned call."""
    T, B, nc = kw["cur_u"].shape
    ns = kw["x_init"].shape[1]
    args = [dev(kw[k], dt) for k in ("x_init", "C", "c", "F", "f", "cur_x", "cur_u")]
    if T == 1:
        args[3], args[4] = torch.empty(0, B, ns, ns + nc, dtype=dt, device=DEV), None
    opts = options(kw, dt, nominal_on_dynamics=vouch)
    out_x = torch.full((T, B, ns), float("nan"), dtype=dt, device=DEV)
    out_u = torch.full((T, B, nc), float("nan"), dtype=dt, device=DEV)
    plan = be.plan_step(*args, opts, impl=impl, out_x=out_x, out_u=out_u)
    r = {k: host(v) for k, v in plan().items() if torch.is_tensor(v)}
    g = be.lqr_step(*args, opts, want_gains=True, impl=impl)
    torch.cuda.synchronize()
    r["K"], r["k"] = host(g["K"]), host(g["k"])
    for k in ("new_x", "new_u", "costs", "alphas", "status"):
        np.testing.assert_array_equal(host(g[k]), r[k], err_msg="planned and unplanned call: " + k)
    return r


def hold(r, o, dt, keep=None, what=""):
    """Every output against the oracle at the device tolerances (module docstring)."""
    B = len(o["costs"])
    keep = np.ones(B, bool) if keep is None else keep
    f64 = dt == F64
    tol = dict(rtol=1e-9, atol=1e-10) if f64 else dict(rtol=1e-3, atol=1e-4)
    same = np.isclose(U.sel(r, "alphas", keep), o["alphas"], rtol=1e-9 if f64 else 1e-5)
    assert (~same).sum() <= (0 if f64 else 1), (what, U.sel(r, "alphas", keep), o["alphas"])
    for k in ("new_x", "new_u"):
        np.testing.assert_allclose(U.sel(r, k, keep)[:, same], o[k][:, same], err_msg="%s %s" % (what, k), **tol)
    np.testing.assert_allclose(U.sel(r, "costs", keep)[same], o["costs"][same], err_msg=what, **(tol if f64 else dict(rtol=2e-4)))
    np.testing.assert_allclose(U.sel(r, "old_costs", keep), o["old_costs"], err_msg=what, **(tol if f64 else dict(rtol=1e-5)))
    for k in ("full_du_norm", "alpha_du_norm"):
        # (full_du_norm is the alpha = 1 trial's whatever the search then takes; alpha_du_norm the accepted trial's)
        sl = same if k == "alpha_du_norm" else np.ones(len(same), bool)
        np.testing.assert_allclose(U.sel(r, k, keep)[sl], o[k][sl], err_msg="%s %s" % (what, k), **(tol if f64 else dict(rtol=1e-3, atol=1e-4)))
    for k in ("K", "k"):
        np.testing.assert_allclose(U.sel(r, k, keep), o[k], err_msg="%s %s" % (what, k), **tol)


def flags_off_nominal(verifier, mode):
    """include/mpc_lqr.h, the status word: the 12/4 kernels verify x_0 = x_init and the dynamics in every mode, the 32/8 kernels in
    the unconstrained step; the others never report bit 4."""
    return verifier == "dpp16" or (verifier == "mfma40" and mode == "free")


@pytest.mark.parametrize("mode,T,with_f", CASES, ids=["%s-T%d-%s" % (m, T, "f" if wf else "nof") for m, T, wf in CASES])
@pytest.mark.parametrize("impl,dt,ns,nc,B,fam,verifier", ROWS, ids=ROW_IDS)
def test_bare_call_on_a_nominal_off_x_init(be, impl, dt, ns, nc, B, fam, verifier, mode, T, with_f):
    # (mpc_lqr_impl_supported answers for a forced kernel; impl 0 picks one itself and takes every shape)
    assert impl == 0 or be.impl_supported(ns, nc, dt, impl), "impl %d must take %d/%d" % (impl, ns, nc)
    npdt = np.float32 if dt == F32 else np.float64
    kinds = U.kinds_of(B, rot=S.rot_of(mode, T, with_f))
    kw, off = U.make_batch(S.seed_of(ns, nc, B, mode, T, with_f), ns, nc, T, B, mode, with_f, kinds, npdt)
    o = U.oracle(kw)
    r = run_step(be, kw, dt, impl)
    print("impl", impl, npdt.__name__, ns, nc, mode, "T", T, "status", r["status"].tolist() if B <= 9 else sorted(set(r["status"].tolist())),
          "max |new_x - oracle| on the off-nominal problems", float(np.abs(r["new_x"][:, off] - o["new_x"][:, off]).max()),
          "costs kernel / oracle", r["costs"][off][:3].tolist(), o["costs"][off][:3].tolist())
    hold(r, o, dt, what="impl %d %s" % (impl, mode))
    np.testing.assert_array_equal(r["new_x"][0], kw["x_init"].astype(npdt))
    assert (r["status"] & ST_NONFINITE == 0).all()
    want = off if flags_off_nominal(verifier, mode) else np.zeros(B, bool)
    assert ((r["status"] & ST_OFF) != 0).tolist() == want.tolist(), (r["status"], kinds)


@pytest.mark.parametrize("impl,dt,ns,nc,B,fam,verifier", ROWS, ids=ROW_IDS)
def test_vouched_control_row(be, impl, dt, ns, nc, B, fam, verifier):
    """Every problem on its nominal, vouched for and bare: the oracle's numbers, no bit 4."""
    npdt = np.float32 if dt == F32 else np.float64
    for mode in ("free", "box"):
        kw, off = U.make_batch(S.seed_of(ns, nc, B, mode, 6, True), ns, nc, 6, B, mode, True, None, npdt)
        o = U.oracle(kw)
        for vouch in (True, False):
            r = run_step(be, kw, dt, impl, vouch=vouch)
            hold(r, o, dt, what="impl %d %s vouch=%s" % (impl, mode, vouch))
            assert (r["status"] & (ST_NONFINITE | ST_OFF) == 0).all()


# The poisoned batches run on the kernels the CPU emulator has run them on (impl 2..9, and impl 0 where it picks one of those: its
# gated second launch of the generic kernels solves only problems flagged MPC_ST_C_ASYMMETRIC, asserted clear below).  impl 1 is
# left out: the generic kernels' pnqp bookkeeping has not been audited for indices derived from float comparisons.
POISON_ROWS = [(r, i) for r, i in zip(ROWS, ROW_IDS) if r[0] != 1]


@pytest.fixture(scope="module")
def clean_runs(be):
    cache = {}

    def get(impl, dt, ns, nc, B, mode):
        key = (impl, dt, ns, nc, mode)
        if key not in cache:
            npdt = np.float32 if dt == F32 else np.float64
            kw, _ = U.make_batch(S.seed_of(ns, nc, B, mode, 6, True), ns, nc, 6, B, mode, True, None, npdt)
            cache[key] = (kw, U.oracle(kw), run_step(be, kw, dt, impl))
        return cache[key]
    return get


@pytest.mark.parametrize("mode,pname", U.POISON_CASES, ids=["%s-%s" % c for c in U.POISON_CASES])
@pytest.mark.parametrize("impl,dt,ns,nc,B,fam,verifier", [r for r, _ in POISON_ROWS], ids=[i for _, i in POISON_ROWS])
def test_poisoned_problems_are_flagged_and_their_batch_mates_untouched(be, clean_runs, impl, dt, ns, nc, B, fam, verifier, mode, pname):
    """(a) - (d) of tests/test_emu_unvouched.py's test of the same name, on the device."""
    kw0, o0, r0 = clean_runs(impl, dt, ns, nc, B, mode)
    who = U.special_problems(B)
    kw = U.poison(kw0, pname, who, big=1e30 if dt == F32 else 1e200)
    healthy = np.ones(B, bool)
    healthy[who] = False
    r = run_step(be, kw, dt, impl)
    assert (r["status"] & ST_ASYM == 0).all()          # (so impl 0's gated launch of the generic kernels solved nothing)
    assert ((r["status"] & ST_NONFINITE) != 0).tolist() == (~np.isfinite(r["costs"])).tolist(), (r["status"], r["costs"])      # (a)
    flagged = (r["status"][who] & ST_NONFINITE) != 0                                                                            # (d)
    if (fam, mode, pname) in U.FINITE_AND_UNFLAGGED:
        assert not flagged.any()
    else:
        assert flagged.all(), (r["status"][who], r["costs"][who])
    oh = {k: (U.sel(o0, k, healthy) if isinstance(v, np.ndarray) else v) for k, v in o0.items()}
    hold(r, oh, dt, keep=healthy, what="impl %d %s %s" % (impl, mode, pname))                                                  # (b)
    wave_mate_of_off = np.zeros(B, bool)                                                                                        # (c)
    if verifier == "dpp16":
        for b in np.nonzero((r["status"] & ST_OFF) != 0)[0]:
            wave_mate_of_off[4 * (b // 4):4 * (b // 4) + 4] = True
    for key in U.OUTPUTS + ("status", "qp_iters"):
        keep = healthy & ~wave_mate_of_off if key == "costs" else healthy
        np.testing.assert_array_equal(U.sel(r, key, keep), U.sel(r0, key, keep), err_msg=key)


# ---------------------------------------------------------------------------------------------------------------------------
# The other ways in
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,ns,nc,B", [(F32, 12, 4, 9), (F32, 13, 4, 3), (F64, 21, 4, 3)])
def test_sweep_and_rollout_pair_on_a_shifted_x_init(be, dt, ns, nc, B):
    """mpc_lqr_sweep + mpc_lqr_rollout (what a step with a true cost / true dynamics of its own takes)."""
    npdt = np.float32 if dt == F32 else np.float64
    for mode in ("free", "box"):
        kw, off = U.make_batch(S.seed_of(ns, nc, B, mode, 6, True), ns, nc, 6, B, mode, True, U.kinds_of(B, rot=S.rot_of(mode, 6, True)), npdt)
        o = U.oracle(kw)
        args = [dev(kw[k], dt) for k in ("x_init", "C", "c", "F", "f", "cur_x", "cur_u")]
        opts = options(kw, dt)
        sw = be.lqr_sweep(args[0], args[1], args[2], args[3], args[5], args[6], opts)
        ro = be.lqr_rollout(*args, sw["K"], sw["k"], opts, old_costs=sw["old_costs"])
        torch.cuda.synchronize()
        r = {k: host(v) for k, v in ro.items() if torch.is_tensor(v)}
        r.update(K=host(sw["K"]), k=host(sw["k"]), old_costs=host(sw["old_costs"]))
        hold(r, o, dt, what="sweep + rollout %s" % mode)
        np.testing.assert_array_equal(r["new_x"][0], kw["x_init"].astype(npdt))


def test_network_rollout_on_a_shifted_x_init(be):
    """mlp_rollout at (6, 2, [16, 16]), x_init off current_x[0] on some problems: against oracle/env_oracle.py's float64 rollout
    through the same network, by the method and numbers of tests/test_gpu_nn.py::test_network_rollout_and_linearisation_at_full_batches."""
    from oracle import env_oracle as E
    from oracle import lqr_oracle as O
    from test_gpu_fullsize import strict_step_check
    from test_gpu_nn import f32, random_net, spec_of
    ns, nc, hidden, B, T = 6, 2, [16, 16], 37, 6
    net = random_net(ns, nc, hidden, "sigmoid", True, seed=ns * 100 + nc, scale=0.8)
    sp = spec_of(net)
    rng = np.random.RandomState(B)
    n = ns + nc
    x0 = rng.randn(B, ns)
    u0 = np.clip(0.3 * rng.randn(T, B, nc), -0.5, 0.5)
    A = rng.randn(T, B, n, n)
    C = np.einsum("tbki,tbkj->tbij", A, A) + 0.1 * np.eye(n)
    c = rng.randn(T, B, n)
    xs = E.traj(E.MLP, x0, u0, net)
    scale = 1.0 + np.abs(xs).max()
    Fl, fl = E.linearize(E.MLP, xs[:-1].reshape(-1, ns), u0[:-1].reshape(-1, nc), net)
    Fl, fl = Fl.reshape(T - 1, B, ns, n), fl.reshape(T - 1, B, ns)
    x0 = x0.copy()
    x0[[0, 15, 16, 36]] += np.array([0.5, 1e-3, 0.5, 0.05])[:, None]          # (slots 0 and 15 of the first group, 0 of the second, the tail)
    for lo, hi in ((None, None), (-0.5, 0.5)):
        o = O.lqr_step(x0, C, c, Fl, fl, xs, u0, lo, hi, linesearch_decay=0.2, max_linesearch_iter=6, lockstep=False, return_gains=True)
        nx, nu, costs, full, alphas, trials, old2 = E.rollout_batched(E.MLP, net, x0, C, c, o["K"], o["k"], xs, u0, lo, hi, 0.2, 6)
        o.update(new_x=nx, new_u=nu, costs=costs, alphas=alphas, old_costs=old2, full_du_norm=full)
        r = be.mlp_rollout(f32(x0), f32(C), f32(c), f32(o["K"]), f32(o["k"]), f32(xs), f32(u0), f32(old2),
                           StepOptions(u_lower=lo, u_upper=hi, linesearch_decay=0.2, max_linesearch_iter=6), sp)
        torch.cuda.synchronize()
        print("network rollout", lo, "max |new_x - oracle| on the shifted problems", float(np.abs(host(r["new_x"]) - nx)[:, [0, 15, 16, 36]].max()))
        ties = strict_step_check("nn_shifted_%s" % lo, r, o, B, rtol=1e-3, atol=2e-4 * scale, cost_rtol=1e-3, have_gains=False)
        assert not ties[[0, 15, 16, 36]].any()
        np.testing.assert_allclose(host(r["full_du_norm"])[~ties], full[~ties], rtol=2e-3, atol=2e-4)
        np.testing.assert_array_equal(host(r["new_x"])[0], x0.astype(np.float32))


@pytest.mark.parametrize("dt", [F64, F32])
def test_simulator_as_true_dynamics_on_a_shifted_x_init(be, dt):
    """impl 4 with the shipped pendulum inside its rollout (mpc/lqr_step.py:223-225) and x_init off current_x[0]: against the float64
    rollout through oracle/env_oracle.py's simulator with the oracle's gains, at the numbers of
    tests/test_gpu_slew_planned.py::test_carry_step_equals_the_route_off_step (float64 1e-9; float32 rtol 1e-3 / atol 1e-4)."""
    from oracle import env_oracle as E
    from oracle import lqr_oracle as O
    from mpc._native import EnvSpec, IMPL_TINY
    z = golden("env_pendulum_f64")
    env = EnvSpec(1, torch.from_numpy(z["params"]).to(dt), 0.05, 2.0)
    lo, hi, decay, max_ls = float(z["lower"][0]), float(z["upper"][0]), float(z["decay"][0]), int(z["max_ls"][0])
    x0 = z["x_init"].copy()
    B = x0.shape[0]
    x0[0] += 0.5
    x0[B - 1] += 1e-3
    o = O.lqr_step(x0, z["Q"], z["p"], z["step_F"], z["step_f"], z["step_cur_x"], z["step_cur_u"], lo, hi, linesearch_decay=decay,
                   max_linesearch_iter=max_ls, lockstep=False, return_gains=True)
    nx, nu, costs, full, alphas, _, old = E.rollout_batched(1, z["params"], x0, z["Q"], z["p"], o["K"], o["k"], z["step_cur_x"], z["step_cur_u"],
                                                            lo, hi, decay, max_ls)
    d = lambda a: dev(a, dt)
    r = be.lqr_step(d(x0), d(z["Q"]), d(z["p"]), d(z["step_F"]), d(z["step_f"]), d(z["step_cur_x"]), d(z["step_cur_u"]),
                    StepOptions(u_lower=lo, u_upper=hi, linesearch_decay=decay, max_linesearch_iter=max_ls, true_dynamics=env), impl=IMPL_TINY)
    torch.cuda.synchronize()
    tol = dict(rtol=1e-9, atol=1e-9) if dt == F64 else dict(rtol=1e-3, atol=1e-4)
    same = np.isclose(host(r["alphas"]), alphas, rtol=1e-6)
    assert same.all() if dt == F64 else (~same).sum() <= 1
    np.testing.assert_allclose(host(r["new_u"])[:, same], nu[:, same], **tol)
    np.testing.assert_allclose(host(r["new_x"])[:, same], nx[:, same], **tol)
    np.testing.assert_allclose(host(r["costs"])[same], costs[same], rtol=tol["rtol"])
    np.testing.assert_allclose(host(r["full_du_norm"]), full, **tol)
    np.testing.assert_array_equal(host(r["new_x"])[0], x0.astype(np.float64 if dt == F64 else np.float32))
    assert (host(r["status"]) & (ST_NONFINITE | ST_OFF) == 0).all()


@pytest.mark.parametrize("ns,nc,B", [(12, 4, 9), (13, 4, 3)])
def test_lqrstep_module_with_current_x_off_x_init(be, ns, nc, B):
    """LQRStep(...)(x_init, C, c, F, f), the autograd node a user calls, with current_x[0] != x_init: the oracle's trajectory."""
    from mpc.lqr_step import LQRStep
    from mpc.mpc import LinDx, QuadCost
    for mode in ("free", "box"):
        kw, off = U.make_batch(S.seed_of(ns, nc, B, mode, 6, True), ns, nc, 6, B, mode, True, U.kinds_of(B, rot=S.rot_of(mode, 6, True)), np.float32)
        o = U.oracle(kw)
        p = {k: dev(kw[k], F32) for k in ("x_init", "C", "c", "F", "f", "cur_x", "cur_u")}
        step = LQRStep(ns, nc, 6, u_lower=kw.get("u_lower"), u_upper=kw.get("u_upper"), true_cost=QuadCost(p["C"], p["c"]),
                       true_dynamics=LinDx(p["F"], p["f"]), current_x=p["cur_x"], current_u=p["cur_u"])
        with torch.no_grad():
            out = step(p["x_init"], p["C"], p["c"], p["F"], p["f"])
        torch.cuda.synchronize()
        new_x, new_u = host(out[0]), host(out[1])
        costs = out[3].costs if hasattr(out[3], "costs") else out[3]
        np.testing.assert_allclose(host(costs), o["costs"], rtol=2e-4, err_msg=mode)
        np.testing.assert_allclose(new_x, o["new_x"], rtol=1e-3, atol=1e-4, err_msg=mode)
        np.testing.assert_allclose(new_u, o["new_u"], rtol=1e-3, atol=1e-4, err_msg=mode)
        np.testing.assert_array_equal(new_x[0], kw["x_init"].astype(np.float32))
