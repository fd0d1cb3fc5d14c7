"""The resident-F build of the mode-0 12/4 step (csrc/lqr_dpp16_body.h, -DMPC_DPP16_RESIDENT; the library's lqr_dpp16_res.o) against
the two-slot-ring build it is routed in place of, on the CPU emulator: the same arithmetic in the same order, so EVERY output
compares equal bit for bit (+-0 alike, NaN where NaN) -- and the oracle agrees at the tolerances the 12/4 kernel's emulator tests
already use (tests/test_emu_unvouched.py: TOL["dpp"]).

What differs between the builds is where the rollouts find F: the sweep copies the F blocks of up to seven timesteps LDS -> LDS behind
the ring (which timesteps depends on the wavefront: res_slot), the identity-priced rollout passes read them there and alias the
stage's three F instructions to the record's lines.  Both placements the Makefile names are emulated (stride 7 from t = 0, the shipped
one; stride 4 over the last 28 entries).  B = 70 is 18 wavefronts: every residency phase of both strides, and a ragged last
wave; T - 1 <= 7 keeps the whole horizon; T = 64 is the last horizon of the register-resident gains."""
import ctypes
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import unvouched_cases as U

ST_OFF = 4
T_ALL = (1, 2, 8, 9, 29, 30, 50, 64)
B_ALL = (1, 5, 70)
PLACEMENTS = {"tail4": ["-DMPC_DPP16_RES_T0=-28", "-DMPC_DPP16_RES_STRIDE=4"], "even7": ["-DMPC_DPP16_RES_T0=0", "-DMPC_DPP16_RES_STRIDE=7"]}
SHIP, OTHER = "even7", "tail4"          # the placement csrc/lqr_dpp16_body.h defaults to, and the other one
KEYS = ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alpha_du_norm", "alphas", "qp_iters", "status", "K", "k")


def _build_resident(emu, name):
    """tests/emu/emu_mfma16.cpp as emu_backend.build(ring2=True) compiles it, plus -DMPC_DPP16_RESIDENT (and the placement)."""
    here = os.path.dirname(os.path.abspath(emu.__file__))
    so = os.path.join(here, "emu", "libemu_mfma16_res_%s.so" % name)
    src = os.path.join(here, "emu", "emu_mfma16.cpp")
    csrc = os.path.join(here, "..", "mpc.pytorch_amd", "csrc")
    deps = [src, os.path.abspath(__file__)] + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        cxx = "/opt/rocm/lib/llvm/bin/clang++"
        if not os.path.exists(cxx):
            cxx = shutil.which("clang++")
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-DMPC_DPP16_NSTAGE=2", "-DMPC_KKT16_NSTAGE=2",
                               "-DMPC_MFMA40_SWEEP_NSTAGE=2", "-DMPC_DPP16_RESIDENT"] + PLACEMENTS[name] + ["-o", tmp, src])
        os.replace(tmp, so)
    return so


@pytest.fixture(scope="module")
def builds(emu_libs):
    """{"parent": the two-slot-ring library as the suite builds it today, placement name: the resident build}"""
    emu = emu_libs
    with ThreadPoolExecutor(max_workers=2) as ex:
        sos = list(ex.map(lambda n: _build_resident(emu, n), list(PLACEMENTS)))
    libs = {"parent": emu.lib_ring2()}
    for name, so in zip(PLACEMENTS, sos):
        L = ctypes.CDLL(so)
        L.emu_lqr_step_dpp16.argtypes = libs["parent"].emu_lqr_step_dpp16.argtypes
        libs[name] = L
    return emu, libs


def run(builds, which, kw, dma_late=True, vouch=False, **opt):
    """One emulated step on build `which` (emu_backend.lqr_step's "dpp16_ring2" row, pointed at that library)."""
    emu, libs = builds
    keep = emu._LIB2
    emu._LIB2 = libs[which]
    try:
        return emu.lqr_step(kernel="dpp16_ring2", dma_late=dma_late, nominal_on_dynamics=vouch, **kw, **opt)
    finally:
        emu._LIB2 = keep


def same_bits(a, b, what):
    for key in KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), "%s: %s differs" % (what, key)      # (== : +0 and -0 alike)


def kinds_for(B):
    """Where the off-nominal problems sit: in-wave positions 0 and 3, a full healthy wave between, the ragged tail's only problems."""
    kinds = ["ok"] * B
    if B == 1:
        kinds[0] = "both"
    elif B == 5:
        kinds[0], kinds[4] = "x0_small", "both"
    else:
        kinds[0], kinds[3], kinds[41], kinds[69] = "x0_big", "x0_small", "both", "both"
    return kinds


def _seed(T, B, with_f, case):
    return 7000 + 100 * T + 3 * B + int(with_f) + 11 * len(case)


def _batch(T, B, with_f, case):
    kinds = kinds_for(B) if case == "off_nominal" else None
    kw, off = U.make_batch(_seed(T, B, with_f, case), 12, 4, T, B, "free", with_f, kinds)
    return kw, off


def shapes(T_all=T_ALL):
    """Every (T, B) with f and without for B = 1 and 5; B = 70 -- 18 emulated wavefronts, 5 to 7 s a run at the long horizons -- with f at
    every other horizon and without at the rest, and on fewer builds (wide() below)."""
    return [(T, B, wf) for T in T_all for B in B_ALL for wf in ((True, False) if B <= 5 else (T_ALL.index(T) % 2 == 0,))]


def wide(B):
    return B <= 5


SHAPE_IDS = lambda v: ["T%d-B%d-%s" % (T, B, "f" if wf else "nof") for T, B, wf in v]


@pytest.mark.parametrize("T,B,with_f", shapes(), ids=SHAPE_IDS(shapes()))
def test_resident_equals_ring2_bit_for_bit_and_the_oracle(builds, T, B, with_f):
    """A nominal on the dynamics, vouched (one identity-priced pass, no verification) and bare (the CHECK pass): both placements
    against the parent build bit for bit, DMA data landing as late as the counted waits allow and (the shipped placement) as early
    as legal -- a correct kernel gives the same bits either way; the parent against the oracle."""
    from test_emu_unvouched import TOL, compare
    kw, _ = _batch(T, B, with_f, "plain")
    for vouch in (True, False):
        ref = run(builds, "parent", kw, vouch=vouch)
        assert (ref["status"] & (2 | ST_OFF) == 0).all()
        same_bits(run(builds, SHIP, kw, vouch=vouch), ref, "shipped vouch=%s late" % vouch)
        if vouch or wide(B):
            same_bits(run(builds, OTHER, kw, vouch=vouch), ref, "other vouch=%s late" % vouch)
        if vouch and wide(B):
            same_bits(run(builds, SHIP, kw, vouch=vouch, dma_late=False), ref, "shipped vouch=%s early" % vouch)
            compare(ref, U.oracle(kw), TOL["dpp"][0], what="T%d B%d" % (T, B))      # (one reference call per problem: the small batches)


@pytest.mark.parametrize("T,B,with_f", shapes(), ids=SHAPE_IDS(shapes()))
def test_resident_off_nominal_passes(builds, T, B, with_f):
    """A bare call whose nominal is off x_init (x_init != current_x[0]) and off the dynamics later: the CHECK pass on resident F
    finds it, the wave re-prices from C on the general ring (the DIRECT pass, no residency) -- bit for bit the parent, the status
    bit on exactly the shifted problems, and the oracle's answer."""
    from test_emu_unvouched import TOL, compare
    kw, off = _batch(T, B, with_f, "off_nominal")
    ref = run(builds, "parent", kw)
    assert ((ref["status"] & ST_OFF) != 0).tolist() == off.tolist()
    same_bits(run(builds, SHIP, kw), ref, "shipped late")
    if wide(B):
        same_bits(run(builds, OTHER, kw), ref, "other late")
        same_bits(run(builds, SHIP, kw, dma_late=False), ref, "shipped early")
        compare(ref, U.oracle(kw), TOL["dpp"][0], what="T%d B%d" % (T, B))


# the state block of every stage cost loses this multiple of the identity: not convex in the state any more (Quu stays positive definite)
BACKOFF_SHIFT = 16.0


def backoff_batch(T, B, with_f, attempt=0):
    kw, _ = U.make_batch(_seed(T, B, with_f, "backoff") + 1000 * attempt, 12, 4, T, B, "free", with_f, None)
    kw["C"] = kw["C"].copy()
    kw["C"][:, :, :12, :12] -= BACKOFF_SHIFT * np.eye(12)
    return kw


@pytest.mark.parametrize("T,B,with_f", shapes(T_ALL[1:]), ids=SHAPE_IDS(shapes(T_ALL[1:])))
def test_resident_line_search_backs_off(builds, T, B, with_f):
    """A stage cost that is not convex in the state: the full step makes some problems worse, their rows go through alpha = decay,
    the multi-trial pass and the replay -- every one of them an identity-priced pass on resident F.  Vouched and bare, bit for bit
    the parent; on the small batches at the short horizons the accepted step sizes are the oracle's, and its costs at the tolerance
    the suite gives non-convex problems (test_emulated_padded_mfma40_line_search_and_off_dynamics_nominal: rtol 4e-3, atol 1e-2)."""
    opt = dict(linesearch_decay=0.5, max_linesearch_iter=8)
    for attempt in range(12):
        kw = backoff_batch(T, B, with_f, attempt)
        ref = run(builds, "parent", kw, vouch=True, **opt)
        if (ref["alphas"] < 1).any() and np.isfinite(ref["costs"]).all():
            break
    else:
        assert False, "no seed made the line search back off"
    same_bits(run(builds, SHIP, kw, vouch=True, **opt), ref, "shipped vouched late")
    if wide(B):
        same_bits(run(builds, OTHER, kw, vouch=True, **opt), ref, "other vouched late")
        same_bits(run(builds, SHIP, kw, vouch=True, dma_late=False, **opt), ref, "shipped vouched early")
        same_bits(run(builds, SHIP, kw, vouch=False, **opt), run(builds, "parent", kw, vouch=False, **opt), "shipped bare late")
        if T <= 9:
            o = U.oracle(dict(kw, **opt))
            np.testing.assert_allclose(ref["alphas"], o["alphas"], rtol=1e-6)
            np.testing.assert_allclose(ref["costs"], o["costs"], rtol=4e-3, atol=1e-2)


def test_resident_lds_budget_and_placements():
    """The ring plus seven blocks fits a wavefront's quarter of the CU's LDS, and the kernel source carries both placements' switches."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mpc.pytorch_amd", "csrc")
    body = open(os.path.join(csrc, "lqr_dpp16_body.h")).read()
    assert "RES_STAGES = 7" in body and "LDS_RES_TOTAL <= 40960" in body
    assert 2 * 9216 + 7 * 3072 <= 40960
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "lqr_dpp16_res.o" in mk and "-DMPC_DPP16_RESIDENT" in mk
