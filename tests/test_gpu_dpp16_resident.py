"""GPU: the resident-F build of the mode-0 12/4 step (lqr_dpp16_res.o, routed for batches of at most one wavefront per SIMD) against
the two-slot-ring build it replaces (MPC_DPP16_RESIDENT=0), in one process: the same arithmetic in the same order, so new_x, new_u,
costs, alphas, both du norms and the status word compare EQUAL.  Every output buffer is pre-filled with NaN (-1 in the status word).

The shapes and cases are those of tests/test_emu_dpp16_resident.py -- T in {1, 2, 8, 9, 29, 30, 50, 64} x B in {1, 5, 70}, with f and
without, vouched and bare; a nominal off x_init and off the dynamics (the re-pricing pass on the general ring); a stage cost that is
not convex in the state (line searches that back off: the multi-trial pass and the replay) -- plus the headline shape once.
mpc_lqr_resident_launches tells which launcher a call took: B = 4100, more wavefronts than SIMDs, must take the old one."""
import numpy as np
import pytest
import torch

import unvouched_cases as U
from mpc import _native
from mpc._native import StepOptions, IMPL_DPP16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("new_x", "new_u", "costs", "old_costs", "alphas", "full_du_norm", "alpha_du_norm", "status", "qp_iters")
T_ALL = (1, 2, 8, 9, 29, 30, 50, 64)
B_ALL = (1, 5, 70)


@pytest.fixture(scope="module")
def be():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return _native.HipBackend()


def step(be, p, monkeypatch, resident, vouch, **opt):
    """One step with the switch set; -> (outputs cloned off NaN-filled buffers, how many launches took the resident build)."""
    monkeypatch.setenv("MPC_DPP16_RESIDENT", "1" if resident else "0")
    plan = be.plan_step(p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"],
                        StepOptions(nominal_on_dynamics=vouch, **opt), impl=IMPL_DPP16)
    for key in KEYS:
        plan.outputs[key].fill_(float("nan") if plan.outputs[key].dtype.is_floating_point else -1)
    n0 = _native.load().mpc_lqr_resident_launches()
    plan()
    torch.cuda.synchronize()
    return {key: plan.outputs[key].clone() for key in KEYS}, _native.load().mpc_lqr_resident_launches() - n0


def to_dev(kw):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    return {k: t(kw[k]) for k in ("x_init", "C", "c", "F", "f", "cur_x", "cur_u")}


def both(be, p, monkeypatch, vouch, what, want_resident=1, **opt):
    on, n_on = step(be, p, monkeypatch, True, vouch, **opt)
    off, n_off = step(be, p, monkeypatch, False, vouch, **opt)
    assert (n_on, n_off) == (want_resident, 0), (what, n_on, n_off)
    for key in KEYS:
        assert not torch.isnan(off[key]).any() if off[key].dtype.is_floating_point else (off[key] >= 0).all(), (what, key)
        assert torch.equal(on[key], off[key]), "%s: %s differs" % (what, key)
    return on


@pytest.mark.parametrize("T", T_ALL)
def test_resident_equals_ring2_on_device(be, monkeypatch, T):
    from test_emu_dpp16_resident import _batch, backoff_batch
    backed_off = False
    for B in B_ALL:
        for with_f in (True, False):
            p = to_dev(_batch(T, B, with_f, "plain")[0])
            want = 1 if T >= 2 else 0          # (T = 1 has no F: the route keeps it on the two-slot build)
            for vouch in (True, False):
                r = both(be, p, monkeypatch, vouch, "plain T%d B%d f%d vouch%d" % (T, B, with_f, vouch), want)
                assert (r["status"] & 6 == 0).all()
            kw, off = _batch(T, B, with_f, "off_nominal")
            r = both(be, to_dev(kw), monkeypatch, False, "off-nominal T%d B%d f%d" % (T, B, with_f), want)
            assert ((r["status"] & 4) != 0).cpu().numpy().tolist() == off.tolist()
            if T >= 2:
                p = to_dev(backoff_batch(T, B, with_f))
                for vouch in (True, False):
                    r = both(be, p, monkeypatch, vouch, "back-off T%d B%d f%d vouch%d" % (T, B, with_f, vouch), want,
                             linesearch_decay=0.5, max_linesearch_iter=8)
                    backed_off = backed_off or bool((r["alphas"] < 1).any())
    assert backed_off or T < 2, "no line search backed off at T = %d" % T


def test_resident_headline_shape_and_the_batch_beyond_one_wave_per_simd(be, monkeypatch):
    """T = 50, B = 4096 (1024 wavefronts: every SIMD of the device, all residency phases many times over) takes the resident build
    and equals the old one; B = 4100 is one wavefront more than there are SIMDs: the old launcher, whatever the switch says."""
    import bench
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    p = bench.make_problem(12, 4, 50, 4 * simds, torch.float32, DEV, seed=2, u_scale=0.0, clamp=None)
    for vouch in (True, False):
        both(be, p, monkeypatch, vouch, "headline vouch%d" % vouch, 1)
    p = bench.make_problem(12, 4, 50, 4 * simds + 4, torch.float32, DEV, seed=3, u_scale=0.0, clamp=None)
    both(be, p, monkeypatch, True, "one wavefront beyond the SIMDs", 0)
    # the switch unset: the resident build where the launch is bound by its traffic (more than 15/16 of one wavefront per SIMD), the old
    # one where the wavefront's own chain is the launch (half the SIMDs: measured slower there, docs/history/r20.md)
    monkeypatch.delenv("MPC_DPP16_RESIDENT", raising=False)
    for B, want in ((4 * simds, 1), (2 * simds, 0)):
        p = bench.make_problem(12, 4, 50, B, torch.float32, DEV, seed=4, u_scale=0.0, clamp=None)
        plan = be.plan_step(p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"], StepOptions(nominal_on_dynamics=True), impl=IMPL_DPP16)
        n0 = _native.load().mpc_lqr_resident_launches()
        plan()
        torch.cuda.synchronize()
        assert _native.load().mpc_lqr_resident_launches() - n0 == want, B
