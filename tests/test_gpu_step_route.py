"""GPU: tests/golden/step_route_expect.json -- which kernel takes a legal mpc_lqr_step call, written by hand from the ladder of
step_impl (docs/history/r15.md) -- held against the kernels themselves.

For every row that asks for impl 0: the step under impl 0, then the row's expected kernel as a FORCED impl on the same inputs,
every output compared bitwise.  A row whose expected kernel is wrong runs two different kernels, and two kernels do not round
alike.  One pair this cannot tell apart: the exact and the padded instantiation of one kernel (3 / 8 at 12/4, 5 / 7 at 32/8) may
produce identical bits at the exact shape; tests/test_step_route_host.py separates them through mpc_lqr_step_route.  The sweep ring
is not visible here either (a forced impl follows the same ring rule).

Where mpc_lqr_qp_record says the step leaves the solutions k_t of its box QPs in the workspace, that record is compared bitwise
with the k the same step returns when asked for gains.

Only entries that were there before the change are called, so this file runs unchanged on a build of the commit before it:
that run is what validates the hand-written table."""
import ctypes
import functools
import json
import os

import pytest
import torch

from conftest import GOLDEN
from mpc import _native
from mpc._native import StepOptions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("new_x", "new_u", "costs", "old_costs", "full_du_norm", "alpha_du_norm", "alphas", "qp_iters", "status")


def gpu_rows():
    with open(os.path.join(GOLDEN, "step_route_expect.json")) as fh:
        t = json.load(fh)
    return [row for row in (dict(t["defaults"], **r) for r in t["rows"]) if row["gpu"] and row["impl"] == 0]


@pytest.fixture(scope="module")
def be():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return _native.HipBackend()


@functools.lru_cache(maxsize=None)
def problem(ns, nc, T, B, dtype, align):
    """One problem per (shape, sizes, dtype), shared by the rows that use it and never written; align 4: every tensor 4 bytes off
    the 16-byte grid (float32 rows only)."""
    import bench
    p = bench.make_problem(ns, nc, T, B, dtype, DEV, seed=3 + ns + T, u_scale=0.3, clamp=0.4)
    g = torch.Generator().manual_seed(11)
    p["lo"] = (-0.45 - 0.1 * torch.rand(T, B, nc, generator=g)).to(dtype).to(DEV)
    p["hi"] = (0.45 + 0.1 * torch.rand(T, B, nc, generator=g)).to(dtype).to(DEV)
    p["mask"] = (torch.rand(T, B, nc, generator=g) < 0.2).to(torch.uint8).to(DEV)
    if align == 4:
        assert dtype == torch.float32
        for key in ("C", "c", "F", "f", "x_init", "cur_x", "cur_u"):
            buf = torch.empty(p[key].numel() + 4, dtype=dtype, device=DEV)
            p[key] = buf[1:1 + p[key].numel()].view(p[key].shape).copy_(p[key])
            assert p[key].data_ptr() % 16 == 4
    return p


def options(row):
    lo, hi = {"none": (None, None), "scalar": (-0.5, 0.5), "tensor": ("lo", "hi")}[row["bounds"]]
    return lambda p: StepOptions(u_lower=p.get(lo, lo), u_upper=p.get(hi, hi), u_zero_I=p["mask"] if row["mask"] else None,
                                 max_linesearch_iter=row["max_ls"], sweep_only=row["sweep_only"])


def run_step(be, row, impl, gains):
    """mpc_lqr_step on the row's inputs -> (outputs, the workspace as the call saw it, p, o, keep)."""
    ns, nc = row["shape"]
    dtype = torch.float32 if row["dtype"] == "f32" else torch.float64
    T, B = row["T"], row["B"]
    p = problem(ns, nc, T, B, dtype, row["align"])
    L = _native.load()
    prob, keep = be._problem(p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"])
    o, keep_o = options(row)(p).to_struct(T, B, nc, p["C"])
    kw = dict(device=DEV, dtype=dtype)
    res = dict(new_x=torch.zeros(T, B, ns, **kw), new_u=torch.zeros(T, B, nc, **kw))
    res.update((name, torch.zeros(B, **kw)) for name in ("costs", "old_costs", "full_du_norm", "alpha_du_norm", "alphas"))
    res.update(qp_iters=torch.zeros(B, device=DEV, dtype=torch.int32), status=torch.zeros(B, device=DEV, dtype=torch.int32))
    if gains:
        res.update(K=torch.zeros(T, B, nc, ns, **kw), k=torch.zeros(T, B, nc, **kw))
    out = be._bind_outputs(res)
    nbytes = int(L.mpc_lqr_workspace_bytes(ctypes.byref(prob)))
    buf = torch.zeros(nbytes + 16, device=DEV, dtype=torch.uint8)
    ws = {"full": buf[:nbytes], "misaligned": buf[4:4 + nbytes], "none": None}[row["workspace"]]
    if ws is not None:
        assert ws.data_ptr() % 16 == (4 if row["workspace"] == "misaligned" else 0)
    rc = L.mpc_lqr_step(ctypes.byref(prob), ctypes.byref(o), ctypes.byref(out), None if ws is None else ws.data_ptr(),
                        0 if ws is None else nbytes, int(impl), torch.cuda.current_stream().cuda_stream)
    _native._check(rc, "mpc_lqr_step (impl %d)" % impl)
    torch.cuda.synchronize()
    return res, ws, prob, o, (keep, keep_o, p)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


@pytest.mark.parametrize("row", gpu_rows(), ids=lambda row: row["id"])
def test_impl_0_runs_the_kernel_the_table_names(be, row):
    auto, ws, prob, o, _keep = run_step(be, row, 0, row["gains"])
    forced, _, _, _, _keep2 = run_step(be, row, row["kernel"], row["gains"])
    assert torch.isfinite(auto["old_costs"]).all()
    for name in OUTPUTS + (("K", "k") if row["gains"] else ()):
        assert torch.equal(bits(auto[name]), bits(forced[name])), name
    # the record of the box QPs' solutions a later step may start from, where the step keeps one
    if row["bounds"] == "none" or row["gains"] or row["workspace"] != "full" or row["dtype"] != "f32" or row["sweep_only"]:
        return
    off, st, sb = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    if not _native.load().mpc_lqr_qp_record(ctypes.byref(prob), ctypes.byref(o), 0, ctypes.byref(off), ctypes.byref(st), ctypes.byref(sb)):
        assert row["kernel"] not in (3, 5, 7)            # (the kernels that take the hint keep the record)
        return
    nc = row["shape"][1]
    record = ws[off.value:].view(torch.float32).as_strided((row["T"], row["B"], nc), (st.value, sb.value, 1)).clone()
    with_gains, _, _, _, _keep3 = run_step(be, row, 0, True)
    assert torch.equal(bits(record), bits(with_gains["k"]))
