"""The NARROW instantiation of the padded 32/8 kernel (lqr_mfma40_body.h, -DMPC_MFMA40_XT=1: one 16-row state tile, n_state <= 16)
through the wavefront emulator: every output equals the padded instantiation's BITWISE (the second state tile of the padded
kernel holds exact zeros at these shapes, the narrow kernel adds the same numbers in the same order without them; the emulator
is built with contraction off), and both agree with the float64 oracle by the method and tolerances of the padded kernel's own
emulator tests (tests/test_emu_mfma16.py)."""
import numpy as np
import pytest

import emu_backend as E
import emu_narrow as EN

# (n_state, n_ctrl, gather granule): 13/4 and 16/4 are what a 12/4 solve with a slew-rate penalty and its neighbours run at, 16/8
# the widest, 9/6 and 14/3 odd on both sides, 1/1 the smallest; (12,8) and (16,4) again with 16-byte gathers
SHAPES = [(13, 4, 4), (16, 4, 4), (16, 8, 4), (9, 6, 4), (14, 3, 4), (1, 1, 4), (12, 8, 16), (16, 4, 16)]
OUTPUTS = ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alpha_du_norm", "alphas", "qp_iters", "status", "K", "k")


def _problem(rng, ns, nc, T, B, u_scale=0.3, clamp=None):
    from oracle import lqr_oracle as O
    n = ns + nc
    A = rng.standard_normal((T, B, n, n))
    C = np.einsum("tbji,tbjk->tbik", A, A) + 0.1 * np.eye(n)
    c = rng.standard_normal((T, B, n))
    F = np.concatenate((np.eye(ns) + 0.2 * rng.standard_normal((max(T - 1, 0), B, ns, ns)) / np.sqrt(ns),
                        rng.standard_normal((max(T - 1, 0), B, ns, nc)) / np.sqrt(ns)), 3)
    f = 0.1 * rng.standard_normal((max(T - 1, 0), B, ns))
    x_init = rng.standard_normal((B, ns))
    cur_u = u_scale * rng.standard_normal((T, B, nc))
    if clamp is not None:
        cur_u = np.clip(cur_u, -clamp, clamp)
    cur_x, _ = O.traj_cost(x_init, cur_u, F, f)
    return dict(x_init=x_init, C=C, c=c, F=F, f=f, cur_x=cur_x, cur_u=cur_u)


def _same_bits(a, b):
    """equal bit for bit, +0 and -0 alike"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))).all())
    return bool((a == b).all())


def _both(pad, kw, opt, vouch, full, c_symmetric=None):
    """the same call on the narrow and on the padded library of this gather granule; asserts every output bitwise equal"""
    o = dict(opt, nominal_on_dynamics=vouch, c_symmetric=vouch if c_symmetric is None else c_symmetric, full=full)
    rn = EN.step(EN.lib(pad), **kw, **o)
    rp = EN.step(E.lib_pad(pad), **kw, **o)
    for key in OUTPUTS:
        assert _same_bits(rn[key], rp[key]), (key, pad, vouch, full, np.abs(rn[key].astype(np.float64) - rp[key]).max())
    return rn, rp


@pytest.mark.parametrize("ns,nc,pad", SHAPES)
def test_narrow_unconstrained_equals_padded_and_oracle(ns, nc, pad):
    """T = 6, B = 2 (the padded kernel's own emulator test): vouched (lean rollout) and bare (nominal verified in the sweep, C
    tested), whole step and sweep alone."""
    from oracle import lqr_oracle as O
    kw = _problem(np.random.default_rng(100 * ns + nc), ns, nc, 6, 2, u_scale=0.0)
    o = O.lqr_step(lockstep=False, return_gains=True, **kw)
    for vouch in (False, True):
        for full in (True, False):
            rn, rp = _both(pad, kw, {}, vouch, full)
            for r in (rn, rp):
                np.testing.assert_allclose(r["K"], o["K"], rtol=1e-3, atol=2e-5)
                np.testing.assert_allclose(r["k"], o["k"], rtol=1e-3, atol=2e-5)
                np.testing.assert_allclose(r["old_costs"], o["old_costs"], rtol=1e-5)
                if full:
                    np.testing.assert_allclose(r["new_x"], o["new_x"], rtol=1e-3, atol=1e-4)
                    np.testing.assert_allclose(r["new_u"], o["new_u"], rtol=1e-3, atol=1e-4)
                    np.testing.assert_allclose(r["costs"], o["costs"], rtol=1e-4)
                    np.testing.assert_allclose(r["full_du_norm"], o["full_du_norm"], rtol=1e-3, atol=1e-4)
                    assert (r["status"] & ~32 == 0).all() and ((r["status"] & 32 != 0).all() == (not vouch))
                else:
                    assert np.isnan(r["new_x"]).all() and np.isnan(r["new_u"]).all() and np.isnan(r["costs"]).all()


@pytest.mark.parametrize("case", ["bounded", "tensor_bounds", "delta_u", "masked", "T1", "T2", "no_f"])
@pytest.mark.parametrize("ns,nc,pad", SHAPES)
def test_narrow_constrained_modes_equal_padded_and_oracle(ns, nc, pad, case):
    """Scalar and tensor box, delta_u, u_zero_I, the short horizons and a problem without f at T = 5, B = 2 (the padded kernel's
    own emulator test): vouched (priced from the sweep's record) and bare (priced from C), whole step and sweep alone."""
    from oracle import lqr_oracle as O
    T = {"T1": 1, "T2": 2}.get(case, 5)
    B = 2
    rng = np.random.default_rng(7 * ns + nc + len(case))
    kw = _problem(rng, ns, nc, max(T, 2), B, u_scale=0.3, clamp=0.4)
    if T == 1:
        kw = {k: (v[:1] if k in ("C", "c", "cur_u") else (v[:0] if k in ("F", "f") else v)) for k, v in kw.items()}
        kw["cur_x"] = kw["x_init"][None].copy()
    if case == "no_f":
        kw["f"] = None
        kw["cur_x"], _ = O.traj_cost(kw["x_init"], kw["cur_u"], kw["F"], None)
    opt = dict(linesearch_decay=0.5, max_linesearch_iter=6)
    if case == "tensor_bounds":
        opt.update(u_lower=-0.5 - rng.random((T, B, nc)), u_upper=0.5 + rng.random((T, B, nc)))
    elif case == "delta_u":
        opt.update(u_lower=-0.5, u_upper=0.5, delta_u=0.1)
    elif case == "masked":
        opt.update(u_zero_I=rng.random((T, B, nc)) < 0.35)
    else:
        opt.update(u_lower=-0.5, u_upper=0.5)
    o = O.lqr_step(lockstep=False, **kw, **opt)
    for vouch in (True, False):
        _both(pad, kw, opt, vouch, False)
        rn, rp = _both(pad, kw, opt, vouch, True)
        for r in (rn, rp):
            np.testing.assert_allclose(r["alphas"], o["alphas"], rtol=1e-6)
            np.testing.assert_allclose(r["new_x"], o["new_x"], rtol=2e-3, atol=2e-4 * (1 + np.abs(o["new_x"]).max()))
            np.testing.assert_allclose(r["new_u"], o["new_u"], rtol=2e-3, atol=2e-4)
            np.testing.assert_allclose(r["costs"], o["costs"], rtol=2e-4, atol=1e-3)
            np.testing.assert_allclose(r["full_du_norm"], o["full_du_norm"], rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("bounded", [False, True], ids=["unbounded", "bounded"])
@pytest.mark.parametrize("ns,nc,pad", [(13, 4, 4), (16, 4, 16)])
def test_narrow_nonsymmetric_C_is_reported_as_by_the_padded_kernel(ns, nc, pad, bounded):
    """A C that is not symmetric: both instantiations flag MPC_ST_C_ASYMMETRIC (8) on the problem that has it and write the
    same bits everywhere."""
    kw = _problem(np.random.default_rng(3 + ns), ns, nc, 5, 3, u_scale=0.3, clamp=0.4)
    kw["C"][2, 1, 0, ns] += 0.5
    opt = dict(u_lower=-0.5, u_upper=0.5) if bounded else {}
    for full in (True, False):
        rn, _ = _both(pad, kw, opt, True, full, c_symmetric=False)
        assert ((rn["status"] & 8) != 0).tolist() == [False, True, False]
        assert (rn["status"] & 32 != 0).all()


@pytest.mark.parametrize("ns,nc,pad,bounded", [(13, 4, 4, False), (13, 4, 4, True), (16, 4, 16, False)])
def test_narrow_line_search_beyond_the_first_trial(ns, nc, pad, bounded):
    """A non-convex stage cost makes later trials win (the parked second trial's copy, the replay, the analytic search): the
    same winners and the same bits as the padded kernel, and the oracle's step sizes."""
    from oracle import lqr_oracle as O
    for attempt in range(40):
        rng = np.random.default_rng(11 + ns + 1000 * attempt)
        kw = _problem(rng, ns, nc, 6, 3, u_scale=0.3, clamp=0.4 if bounded else None)
        kw["C"][:, :, :ns, :ns] -= (80.0 if bounded else 45.0) * np.eye(ns)
        opt = dict(linesearch_decay=0.5, max_linesearch_iter=8)
        if bounded:
            opt.update(u_lower=-0.5, u_upper=0.5)
        o = O.lqr_step(lockstep=False, **kw, **opt)
        if (o["alphas"] < 1).any() and (not bounded or (o["alphas"] > 0.5 ** 7).all()):
            break
    else:
        assert False, "no seed made the line search backtrack"
    for vouch in (True, False):
        rn, _ = _both(pad, kw, opt, vouch, True)
        np.testing.assert_allclose(rn["alphas"], o["alphas"], rtol=1e-6)
        np.testing.assert_allclose(rn["new_u"], o["new_u"], rtol=2e-2, atol=4e-3 * (1 + np.abs(o["new_u"]).max()))
        np.testing.assert_allclose(rn["costs"], o["costs"], rtol=4e-3, atol=1e-2)


@pytest.mark.parametrize("pad", [4, 16])
def test_the_helper_issues_emu_backends_command_plus_the_one_flag(pad, monkeypatch, tmp_path):
    """emu_backend.build takes no extra flags, so emu_narrow.build repeats its compiler line: held to it here (nothing is compiled)."""
    import os
    import subprocess
    cmds = []
    monkeypatch.setattr(E, "_EMU", str(tmp_path))
    monkeypatch.setattr(subprocess, "check_call", lambda cmd, *a, **k: cmds.append(list(cmd)))
    monkeypatch.setattr(os, "replace", lambda a, b: None)
    E.build(pad=pad)
    EN.build(pad)
    (padded, narrow) = cmds

    def parts(cmd):
        i = cmd.index("-o")
        return cmd[:i], os.path.basename(cmd[i + 2]), cmd[i + 3:]
    assert parts(narrow)[0] == parts(padded)[0] + ["-DMPC_MFMA40_XT=1"] and parts(narrow)[1:] == parts(padded)[1:]
    assert os.path.basename(narrow[narrow.index("-o") + 1]).startswith("libemu_mfma16_narrow%d.so" % pad)
