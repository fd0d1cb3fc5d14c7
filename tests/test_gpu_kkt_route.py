"""The rows of tests/golden/kkt_route_expect.json that torch tensors can express, against the kernels (docs/history/r18.md): the
fused kernel a bound plan reports (HipBackend.kkt_route) and the closed-form kernel of the three-call route
(mpc_lqr_kkt_grads_route on the very tensors used) are the table's; plan_kkt_backward gives no plan where the table has no fused
kernel; plan() is kkt_backward bit for bit; and every route's gradients meet the float64 oracle -- float32 up to n = 64 as
tests/test_gpu_parity.py::test_kkt_backward_wave_kernels holds them (bench.make_problem, 2e-4 of the largest entry), float64 and
n = 65 as tests/test_gpu_generic.py::test_kkt_backward_through_the_generic_gradient_kernel does (its recipe, hold_grads).

[T,B] = [3,5] unless the row names a horizon.  Alignment rows are views one element into their storage (_block_strided keeps
them); `run_row` asks no route, so it also runs on a library from before the queries existed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_generic import O, dev, dynamics, finish, hold_grads, host
from test_kkt_route_host import GRADS, KKT

gpu = pytest.mark.gpu
DEV = "cuda:0"
B = 5
OUTPUTS = ("dx_init", "dC", "dc", "dF", "df", "dx", "du")

with open(os.path.join(GOLDEN, "kkt_route_expect.json")) as _fh:
    _TABLE = json.load(_fh)
ROWS = [dict(_TABLE["defaults"], **dict(row, T=row.get("T", 3), B=B, seed=4100 + i)) for i, row in enumerate(_TABLE["rows"])
        if row.get("gpu", True)]


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mpc import _native
    _native.load()
    return _native.HipBackend()


def one_element_in(t):
    """The same values in a view whose storage starts one element (4 bytes in float32) past an allocation."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def pitched(t, more):
    """The same [T,B,...] values with `more` elements between consecutive problems' blocks."""
    T, Bn, block = t.shape[0], t.shape[1], t[0, 0].numel()
    buf = torch.empty(T * Bn * (block + more), dtype=t.dtype, device=t.device)
    inner = t[0, 0].contiguous().stride()
    v = buf.as_strided(t.shape, (Bn * (block + more), block + more) + inner)
    v.copy_(t)
    return v


def run_row(be, row):
    """-> (oracle arguments, outputs): `plan` / `plain` / `three` = plan(), kkt_backward and the three-call route on the row's views."""
    from mpc._native import StepOptions
    import bench
    ns, nc = row["shape"]
    T, bounded, f32 = row["T"], row["bounds"] == "tensor", row["dtype"] == "f32"
    fwd = StepOptions(u_lower=-0.5, u_upper=0.5) if bounded else StepOptions()
    if row["grads"] == "GENERIC":
        elem, n = 4 if f32 else 8, ns + nc
        rng = np.random.default_rng(row["seed"])
        A = rng.standard_normal((T, B, n, n))
        F, f = dynamics(rng, ns, nc, T, B, True)
        p = finish(elem, rng.standard_normal((B, ns)), np.einsum("tbji,tbjk->tbik", A, A) / n + 0.1 * np.eye(n),
                   rng.standard_normal((T, B, n)), F, f, 0.3 * rng.standard_normal((T, B, nc)))
        p = {k: dev(v) for k, v in p.items()}
        r = be.lqr_step(p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"], fwd, impl=1)
    else:
        p = bench.make_problem(ns, nc, T, B, torch.float32, DEV, seed=row["seed"], u_scale=0.3 if bounded else 0.0,
                               clamp=0.5 if bounded else None)
        r = be.lqr_step(p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"], fwd)
    g = torch.Generator(device="cpu").manual_seed(row["seed"] + 1)
    t = dict(C=p["C"], c=p["c"], F=p["F"], f=p["f"], cur_x=r["new_x"].clone(), cur_u=r["new_u"].clone(),
             dl_dx=torch.randn(T, B, ns, generator=g, dtype=p["C"].dtype).to(DEV), dl_du=torch.randn(T, B, nc, generator=g, dtype=p["C"].dtype).to(DEV),
             lo=torch.full((T, B, nc), -0.5, dtype=p["C"].dtype, device=DEV), hi=torch.full((T, B, nc), 0.5, dtype=p["C"].dtype, device=DEV))
    assert all(nbytes == t[name].element_size() for name, nbytes in row["off"].items()) and set(row["skew"]) <= {"C_sb"}
    for name in row["off"]:
        t[name] = one_element_in(t[name])
    if row["skew"]:
        t["C"] = pitched(t["C"], row["skew"]["C_sb"])
    env = None
    if row["env"]:
        from mpc.env_dx import pendulum
        env = pendulum.PendulumDx().native_env()
        assert env.kind == row["env"]
    opts = StepOptions(u_lower=t["lo"] if bounded else None, u_upper=t["hi"] if bounded else None, c_symmetric=row["symmetric"],
                       true_dynamics=env)
    loose = StepOptions(u_lower=opts.u_lower, u_upper=opts.u_upper, true_dynamics=env)
    args = (t["C"], t["c"], t["F"], t["f"], t["cur_x"], t["cur_u"], t["dl_dx"], t["dl_du"])
    out = dict(plan=None, plain=be.kkt_backward(*args, opts), three=be.kkt_backward(*args, loose))
    plan = be.plan_kkt_backward(*args, opts)
    if plan is not None:
        out["plan"] = plan()
    torch.cuda.synchronize()
    h = lambda a: None if a is None or a.numel() == 0 else host(a).astype(np.float64)
    oracle_args = [h(a) for a in args] + ([-0.5, 0.5] if bounded else [None, None])
    oracle_args[2] = host(t["F"]).astype(np.float64)             # (T = 1: an empty F, not None)
    return oracle_args, args, opts, plan, out


def hold(label, row, g, o64, o32):
    if row["grads"] == "GENERIC":
        return hold_grads(label, g, o64, o32)
    for k in ("dx_init", "dC", "dc", "dF", "df"):
        if o64[k] is None or o64[k].size == 0:
            assert g[k] is None or g[k].numel() == 0, k
            continue
        scale = max(1.0, np.abs(o64[k]).max())
        err = float(np.abs(host(g[k]) / scale - o64[k] / scale).max())
        print("[kkt route] %s %s: %.3g of 2e-4" % (label, k, err))
        np.testing.assert_allclose(host(g[k]) / scale, o64[k] / scale, rtol=0, atol=2e-4, err_msg="%s %s" % (label, k))


@gpu
@pytest.mark.parametrize("row", ROWS, ids=lambda row: row["id"])
def test_a_backward_takes_the_tables_kernels_and_meets_the_oracle(be, row):
    from mpc import _native
    oracle_args, args, opts, plan, out = run_row(be, row)
    fused = KKT[row["kernel"]]
    # the fused kernel: none -> no plan; otherwise the plan's, asked at bind time and again now
    assert (plan is None) == (fused == _native.KKT_NONE)
    if plan is not None:
        assert plan.kernel == fused and be.kkt_route(plan) == fused
        assert out["plan"] is plan.outputs
        for k in OUTPUTS:
            assert (out["plan"][k] is None) == (out["plain"][k] is None), k
            if out["plan"][k] is not None:
                assert torch.equal(out["plan"][k], out["plain"][k]), k
    # the closed-form kernel of the three-call route, on the tensors that call used
    L, _dev, _dims, _kw, (_x, _u, dl_dx, dl_du), _has_f, p, _keep = be._open_kkt(*args)
    three = out["three"]
    ptr = lambda a: None if a is None or a.numel() == 0 else a.data_ptr()
    assert int(L.mpc_lqr_kkt_grads_route(ctypes.byref(p), three["dx"].data_ptr(), three["du"].data_ptr(), dl_dx.data_ptr(), dl_du.data_ptr(),
                                         three["dC"].data_ptr(), three["dc"].data_ptr(), ptr(three["dF"]), ptr(three["df"]),
                                         three["dx_init"].data_ptr())) == GRADS[row["grads"]]
    # every route against the float64 oracle
    o64 = O().kkt_backward(*oracle_args, lockstep=False)
    o32 = None
    if row["grads"] == "GENERIC" and row["dtype"] == "f32":
        o32 = O().kkt_backward(*(a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in oracle_args), lockstep=False)
    hold("%s: kkt_backward" % row["id"], row, out["plain"], o64, o32)
    hold("%s: three calls" % row["id"], row, three, o64, o32)
