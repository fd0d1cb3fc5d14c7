"""GPU: a pre-bound step (HipBackend.plan_step) reports its own route -- HipBackend.step_route(plan), over mpc_lqr_step_route -- and its
record of the box QPs' solutions, row by row of tests/golden/step_route_expect.json.  (tests/test_gpu_step_route.py, which holds that
table against the kernels, calls only entries older than mpc_lqr_step_route; this file is where the new entry meets a device.)"""
import pytest
import torch

from test_gpu_step_route import be, bits, gpu_rows, options, problem, run_step  # noqa: F401  (be: the fixture)

pytestmark = pytest.mark.gpu

PLAN_ROWS = ("12/4 box, small batch: deep ring", "12/4 unconstrained: short ring", "13/4 box", "32/8 box, small batch: three slots",
             "5/3 box", "3/1 scalar box")


@pytest.mark.parametrize("name", PLAN_ROWS)
def test_a_bound_plan_reports_its_route_and_its_record(be, name):
    """HipBackend.step_route(plan) for a pre-bound step is the table's row; HipBackend.qp_record(plan) is the k that step returns when
    asked for gains."""
    row = next(r for r in gpu_rows() if r["id"] == name)
    ns, nc = row["shape"]
    p = problem(ns, nc, row["T"], row["B"], torch.float32, row["align"])
    plan = be.plan_step(p["x_init"], p["C"], p["c"], p["F"], p["f"], p["cur_x"], p["cur_u"], options(row)(p))
    assert be.step_route(plan) == (row["kernel"], row["ring"])
    plan()
    torch.cuda.synchronize()
    record = be.qp_record(plan)
    assert (record is not None) == (row["bounds"] != "none" and row["kernel"] in (3, 5, 7))
    if record is not None:
        with_gains, _, _, _, _keep = run_step(be, row, 0, True)
        assert torch.equal(bits(record), bits(with_gains["k"]))
        assert torch.equal(bits(plan.outputs["new_u"]), bits(with_gains["new_u"]))
