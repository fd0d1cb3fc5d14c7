"""Every emulated step kernel on what a bare LQRStep call may bring and MPC.forward never does:

  * a nominal that is not vouched for (no MPC_OPT_NOMINAL_ON_DYNAMICS) and is OFF x_init -- current_x[0] != x_init, with or without
    a current_x that also leaves the dynamics later.  The reference starts its pass from new_x = [x_init], dx = [zeros_like(x_init)]
    (mpc/lqr_step.py:181-182): dx_0 = 0, new_x[0] = x_init, old_cost the cost of the nominal as given;
  * batches in which some problems are not finite: MPC_ST_NONFINITE on exactly those, the others untouched.

Every problem is held to the float64 oracle (one reference call per problem) at the tolerances the kernel's existing emulator test
uses -- TOL below names the test each row comes from; none is new."""
import numpy as np
import pytest

import unvouched_cases as U

ST_NONFINITE, ST_OFF, ST_TESTED = 2, 4, 32


@pytest.fixture(scope="module")
def emu(emu_libs):
    import emu_backend
    emu_backend.lib()
    return emu_backend


def _atol_scaled(rtol, atol):
    """atol (1 + max |reference|), the 32/8 tests' form"""
    return lambda ref: dict(rtol=rtol, atol=atol * (1 + np.abs(ref).max()))


def _fixed(rtol, atol=0.0):
    return lambda ref: dict(rtol=rtol, atol=atol)


# kernel family -> mode class ("free" | "con") -> output -> tolerance, each from the named test of tests/test_emu_mfma16.py (or
# tests/test_emu_narrow.py).  An output the named tests do not compare takes the tolerance the same test gives its nearest kin
# (alpha_du_norm that of full_du_norm, k that of K), never a wider one.
_DPP = dict(                                           # test_emulated_dpp16_options_against_oracle (trajectory, costs, K, alphas),
    new_x=_fixed(1e-3, 2e-4), new_u=_fixed(1e-3, 2e-4), costs=_fixed(2e-4, 1e-4), K=_fixed(1e-3, 1e-4), k=_fixed(1e-3, 1e-4),
    alphas=_fixed(1e-6),
    old_costs=_fixed(1e-4),                            # test_emulated_dpp16_nominal_off_the_dynamics
    full_du_norm=_fixed(2e-3, 2e-4), alpha_du_norm=_fixed(2e-3, 2e-4))    # test_emulated_dpp16_matches_oracle_and_reference
_M16_FREE = dict(                                      # test_emulated_kernel_matches_oracle_and_reference, unbounded fixtures
    K=_fixed(1e-3, 1e-4), k=_fixed(1e-3, 1e-4), new_x=_fixed(1e-3, 1e-4), new_u=_fixed(1e-3, 1e-4), costs=_fixed(1e-4),
    old_costs=_fixed(1e-4), alphas=_fixed(1e-6), full_du_norm=_fixed(2e-3, 2e-4), alpha_du_norm=_fixed(2e-3, 2e-4))
_M16_CON = dict(_M16_FREE, K=_fixed(1e-3, 1e-3), k=_fixed(1e-3, 1e-3), new_x=_fixed(1e-3, 1e-3), new_u=_fixed(1e-3, 1e-3))   # same test, box-constrained float32 fixtures
_M16_F64_FREE = dict(                                  # test_emulated_float64_kernel_on_the_reference_fixtures
    K=_fixed(1e-9, 1e-9), k=_fixed(1e-9, 1e-9), new_x=_fixed(1e-9, 1e-9), new_u=_fixed(1e-9, 1e-9), costs=_fixed(1e-9),
    old_costs=_fixed(1e-12), alphas=_fixed(1e-12),
    full_du_norm=_fixed(1e-9, 1e-9), alpha_du_norm=_fixed(1e-9, 1e-9))      # (norms of new_u - u: new_u's tolerance)
_M16_F64_CON = dict(_M16_F64_FREE, K=_fixed(1e-6, 1e-6), k=_fixed(1e-6, 1e-6), new_x=_fixed(1e-6, 1e-6), new_u=_fixed(1e-6, 1e-6),
                    full_du_norm=_fixed(1e-6, 1e-6), alpha_du_norm=_fixed(1e-6, 1e-6))
_TINY_F64 = {k: _fixed(1e-10, 1e-11) for k in U.OUTPUTS}              # test_tiny_body_options_against_oracle
_TINY_F32 = dict({k: _fixed(1e-3, 1e-4) for k in U.OUTPUTS}, alphas=_fixed(1e-6))     # test_tiny_body_matches_oracle_and_reference
_WAVE1 = dict({k: _fixed(1e-3, 1e-4) for k in U.OUTPUTS}, alphas=_fixed(1e-6))        # test_wave1_body_matches_oracle
_M40_FREE = dict(                                      # test_emulated_mfma40_verifies_the_nominal_it_is_not_vouched_for
    new_x=_atol_scaled(2e-3, 2e-4), new_u=_atol_scaled(2e-3, 2e-4), costs=_fixed(2e-4, 1e-3), old_costs=_fixed(1e-5), alphas=_fixed(1e-6),
    K=_fixed(1e-3, 2e-5), k=_fixed(1e-3, 2e-5),        # test_emulated_mfma40_sweep_matches_oracle
    full_du_norm=_fixed(1e-3, 1e-4), alpha_du_norm=_fixed(1e-3, 1e-4))      # test_emulated_mfma40_full_step
_M40_CON = dict(_M40_FREE,                             # test_emulated_mfma40_constrained_modes
                K=_atol_scaled(2e-3, 2e-4), k=_fixed(2e-3, 2e-4), new_u=_fixed(2e-3, 2e-4))
_PAD_FREE = dict(                                      # test_emulated_padded_mfma40_unconstrained / test_narrow_unconstrained_equals_padded_and_oracle
    K=_fixed(1e-3, 2e-5), k=_fixed(1e-3, 2e-5), new_x=_fixed(1e-3, 1e-4), new_u=_fixed(1e-3, 1e-4), costs=_fixed(1e-4),
    old_costs=_fixed(1e-5), full_du_norm=_fixed(1e-3, 1e-4), alpha_du_norm=_fixed(1e-3, 1e-4), alphas=_fixed(1e-6))
_PAD_CON = dict(_PAD_FREE,                             # test_emulated_padded_mfma40_constrained_modes / test_narrow_constrained_modes_equal_padded_and_oracle
                new_x=_atol_scaled(2e-3, 2e-4), new_u=_fixed(2e-3, 2e-4), costs=_fixed(2e-4, 1e-3),
                K=_atol_scaled(2e-3, 2e-4), k=_fixed(2e-3, 2e-4))            # (gains: test_emulated_mfma40_constrained_modes)
TOL = {"dpp": (_DPP, _DPP), "m16": (_M16_FREE, _M16_CON), "m16_f64": (_M16_F64_FREE, _M16_F64_CON), "tiny_f64": (_TINY_F64, _TINY_F64),
       "tiny_f32": (_TINY_F32, _TINY_F32), "wave1": (_WAVE1, _WAVE1), "m40": (_M40_FREE, _M40_CON), "pad": (_PAD_FREE, _PAD_CON)}

# (id, emulator kernel, dtype, n_state, n_ctrl, B, tolerance family)
ROWS = [
    ("mfma16-12_4", "mfma16", np.float32, 12, 4, 3, "m16"),
    ("mfma16-5_2", "mfma16", np.float32, 5, 2, 3, "m16"),
    ("mfma16_f64-12_4", "mfma16", np.float64, 12, 4, 3, "m16_f64"),
    ("mfma16_f64-5_2", "mfma16", np.float64, 5, 2, 3, "m16_f64"),
    ("dpp16-12_4", "dpp16", np.float32, 12, 4, 9, "dpp"),
    ("dpp16_ring2-12_4", "dpp16_ring2", np.float32, 12, 4, 9, "dpp"),
    ("dpp16_pad-12_4", "dpp16_pad", np.float32, 12, 4, 9, "dpp"),
    ("dpp16_pad-10_3", "dpp16_pad", np.float32, 10, 3, 9, "dpp"),
    ("tiny-3_1", "tiny", np.float32, 3, 1, 70, "tiny_f32"),
    ("tiny_f64-3_1", "tiny", np.float64, 3, 1, 70, "tiny_f64"),
    ("wave1-3_1", "wave1", np.float32, 3, 1, 9, "wave1"),          # (a DPP row per problem: four problems per wavefront)
    ("mfma40-32_8", "mfma40", np.float32, 32, 8, 3, "m40"),
    ("mfma40_ring2-32_8", "mfma40_ring2", np.float32, 32, 8, 3, "m40"),
    ("mfma40_pad4-13_4", "mfma40_pad4", np.float32, 13, 4, 3, "pad"),
    ("mfma40_pad16-16_4", "mfma40_pad16", np.float32, 16, 4, 3, "pad"),
    ("narrow4-13_4", "narrow4", np.float32, 13, 4, 3, "pad"),
    ("narrow16-16_4", "narrow16", np.float32, 16, 4, 3, "pad"),
]
ROW_IDS = [r[0] for r in ROWS]


def run(emu, kernel, dtype, kw, vouch=False):
    """One emulated step; the narrow pair goes through tests/emu_narrow.py."""
    if kernel.startswith("narrow"):
        import emu_narrow as EN
        return EN.step(EN.lib(int(kernel[6:])), nominal_on_dynamics=vouch, **kw)
    return emu.lqr_step(kernel=kernel, dtype=dtype, dma_late=True, nominal_on_dynamics=vouch, **kw)


def flags_off_nominal(kernel, mode):
    """Does this kernel, in this mode, report MPC_ST_NOMINAL_OFF_DYNAMICS on a bare call (include/mpc_lqr.h, the status word)?
    The 12/4 kernels verify x_0 = x_init and the dynamics in every mode (their rollout is priced by an identity that needs it); the
    32/8 kernels in the unconstrained step only (its line search is decided from the sweep; a constrained bare call is priced
    from C, which needs no premise).  mfma16 and the lane kernels price from C and keep dx_0 = 0 themselves: never."""
    if kernel.startswith("dpp16"):
        return True
    if kernel.startswith(("mfma40", "narrow")):
        return mode == "free"
    return False


def constrained(fam, mode):
    """Which of a family's two tolerance rows a mode takes.  The one-problem-per-wavefront kernel's tests widen theirs only where
    bounds are present (the box QP's stopping rule): its zero-mask rows, which have none, keep the unbounded numbers."""
    return mode != "free" and not (mode == "mask" and fam in ("m16", "m16_f64"))


def compare(r, o, tol, keep=None, what=""):
    keep = np.ones(len(o["costs"]), bool) if keep is None else keep
    for key in U.OUTPUTS:
        got, ref = U.sel(r, key, keep), o[key]
        np.testing.assert_allclose(got, ref, err_msg="%s %s" % (what, key), **tol[key](ref))


def _seed(rid, mode, T, with_f):
    return 1000 * ROW_IDS.index(rid) + 100 * U.MODES.index(mode) + 10 * T + int(with_f)


CASES = [(m, 6, True) for m in U.MODES] + [(m, 6, False) for m in U.MODES] + [("free", 1, True), ("box", 1, True)]


@pytest.mark.parametrize("mode,T,with_f", CASES, ids=["%s-T%d-%s" % (m, T, "f" if wf else "nof") for m, T, wf in CASES])
@pytest.mark.parametrize("rid,kernel,dtype,ns,nc,B,fam", ROWS, ids=ROW_IDS)
def test_bare_call_on_a_nominal_off_x_init(emu, rid, kernel, dtype, ns, nc, B, fam, mode, T, with_f):
    """The nominal matrix: one batch mixing consistent problems, x_init shifted by 0.5, by 1e-3, and current_x[2:] shifted with
    x_init as well, at the in-wave positions where a kernel shares a wave between problems.  Every output of every problem against
    the oracle; MPC_ST_NOMINAL_OFF_DYNAMICS on exactly the off-nominal problems where the kernel verifies, on none where it does not;
    no MPC_ST_NONFINITE anywhere."""
    kinds = U.kinds_of(B, rot=U.rot_of(mode, T, with_f))
    kw, off = U.make_batch(_seed(rid, mode, T, with_f), ns, nc, T, B, mode, with_f, kinds, dtype)
    o = U.oracle(kw)
    r = run(emu, kernel, dtype, kw)
    compare(r, o, TOL[fam][constrained(fam, mode)], what=rid)
    np.testing.assert_array_equal(r["new_x"][0], kw["x_init"].astype(dtype))            # new_x[0] = x_init, :181
    assert (r["status"] & ST_NONFINITE == 0).all()
    want = off if flags_off_nominal(kernel, mode) else np.zeros(B, bool)
    assert ((r["status"] & ST_OFF) != 0).tolist() == want.tolist(), (r["status"], kinds)


@pytest.mark.parametrize("mode", ["free", "box"])
@pytest.mark.parametrize("rid,kernel,dtype,ns,nc,B,fam", ROWS, ids=ROW_IDS)
def test_vouched_control_row(emu, rid, kernel, dtype, ns, nc, B, fam, mode):
    """The control: the same recipe with every problem on its nominal, vouched for (MPC_OPT_NOMINAL_ON_DYNAMICS) -- against the oracle
    at the same tolerances, no bit 4 -- and the bare call on the same batch giving the same accepted steps and no bit 4 either."""
    kw, off = U.make_batch(_seed(rid, mode, 6, True) + 5, ns, nc, 6, B, mode, True, None, dtype)
    assert not off.any()
    o = U.oracle(kw)
    for vouch in (True, False):
        r = run(emu, kernel, dtype, kw, vouch=vouch)
        compare(r, o, TOL[fam][constrained(fam, mode)], what="%s vouch=%s" % (rid, vouch))
        assert (r["status"] & (ST_NONFINITE | ST_OFF) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# Poisoned batches
# ---------------------------------------------------------------------------------------------------------------------------
FINITE_AND_UNFLAGGED, POISON_CASES, special_problems = U.FINITE_AND_UNFLAGGED, U.POISON_CASES, U.special_problems


@pytest.fixture(scope="module")
def clean_runs(emu):
    """(row id, mode) -> (kw, oracle on the whole clean batch, kernel result on it): computed once, shared by the poisons, left
    unchanged."""
    cache = {}

    def get(rid, kernel, dtype, ns, nc, B, mode):
        if (rid, mode) not in cache:
            kw, _ = U.make_batch(_seed(rid, mode, 6, True) + 7, ns, nc, 6, B, mode, True, None, dtype)
            cache[(rid, mode)] = (kw, U.oracle(kw), run(emu, kernel, dtype, kw))
        return cache[(rid, mode)]
    return get


@pytest.mark.parametrize("mode,pname", POISON_CASES, ids=["%s-%s" % c for c in POISON_CASES])
@pytest.mark.parametrize("rid,kernel,dtype,ns,nc,B,fam", ROWS, ids=ROW_IDS)
def test_poisoned_problems_are_flagged_and_their_batch_mates_untouched(emu, clean_runs, rid, kernel, dtype, ns, nc, B, fam, mode, pname):
    """Some problems of a batch made non-finite (wave-mates on purpose: in-wave positions 0, 3 and the tail problem of nine; lanes
    0, 63, 64 of seventy; the middle one of three, for the kernels that give a problem a wavefront of its own).  These are ordinary inputs that must produce a status bit.
      (a) status & 2 is set iff the returned cost is not finite, on every problem;
      (b) the healthy problems meet the oracle run on the healthy problems alone;
      (c) the healthy problems are bit-identical to the same call on the clean batch in every output -- but for `costs` of a
          12/4-kernel problem that shares its wave with an off-dynamics one: the wave prices from C together then (one pass over
          C for the four rows), so the healthy rows' costs are the direct float32 sum instead of the identity's, equal to rounding
          and held by (b) only;
      (d) a poisoned problem comes back finite and unflagged exactly where FINITE_AND_UNFLAGGED says."""
    kw0, o0, r0 = clean_runs(rid, kernel, dtype, ns, nc, B, mode)
    who = special_problems(B)
    kw = U.poison(kw0, pname, who, big=1e30 if dtype == np.float32 else 1e200)
    healthy = np.ones(B, bool)
    healthy[who] = False
    r = run(emu, kernel, dtype, kw)
    # (a)
    assert ((r["status"] & ST_NONFINITE) != 0).tolist() == (~np.isfinite(r["costs"])).tolist(), (r["status"], r["costs"])
    # (d)
    flagged = (r["status"][who] & ST_NONFINITE) != 0
    if (fam, mode, pname) in FINITE_AND_UNFLAGGED:
        assert not flagged.any(), "%s %s %s is flagged now: take it off FINITE_AND_UNFLAGGED and INTEGRATION.md" % (fam, mode, pname)
    else:
        assert flagged.all(), (r["status"][who], r["costs"][who])
    # (b)
    compare(r, {k: (U.sel(o0, k, healthy) if isinstance(v, np.ndarray) else v) for k, v in o0.items()}, TOL[fam][constrained(fam, mode)],
            keep=healthy, what=rid)
    # (c)
    wave_mate_of_off = np.zeros(B, bool)
    if kernel.startswith("dpp16"):
        for b in np.nonzero((r["status"] & ST_OFF) != 0)[0]:
            wave_mate_of_off[4 * (b // 4):4 * (b // 4) + 4] = True
    for key in U.OUTPUTS + ("status", "qp_iters"):
        keep = healthy & ~wave_mate_of_off if key == "costs" else healthy
        np.testing.assert_array_equal(U.sel(r, key, keep), U.sel(r0, key, keep), err_msg="%s %s" % (rid, key))


# ---------------------------------------------------------------------------------------------------------------------------
# The device test's seeds (tests/test_gpu_unvouched.py)
# ---------------------------------------------------------------------------------------------------------------------------
def test_device_seeds_keep_float32_and_float64_on_the_same_alphas():
    """tests/test_gpu_unvouched.py may leave one problem per case out of the trajectory comparison when its line search lands on
    another alpha than the oracle's.  Its recorded seeds are those for which the oracle in float32 and in float64 agree on every
    alpha, so that cap is never what hides a shifted problem: checked here, on the CPU."""
    import unvouched_gpu_seeds as S
    from oracle import lqr_oracle as O
    for (ns, nc, B, mode, T, with_f), seed in sorted(S.SEEDS.items()):
        for kinds in (U.kinds_of(B, rot=S.rot_of(mode, T, with_f)), None):
            kw, _ = U.make_batch(seed, ns, nc, T, B, mode, with_f, kinds, np.float32)
            o64 = O.lqr_step(lockstep=False, **kw)
            o32 = O.lqr_step(lockstep=False, **{k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v)
                                                for k, v in kw.items()})
            np.testing.assert_array_equal(o32["alphas"].astype(np.float64), o64["alphas"], err_msg=str((ns, nc, B, mode, T, with_f, seed)))
