"""CPU-only: the host side of the NNDynamics kernels (csrc/nn_dynamics.hip, nn_param_grad.h) answers what it answered
before it was rewritten around one layout, one validation and one plan per entry point (docs/history/r13.md).

tests/golden/nn_plan_answers.json was recorded from a build of the commit before that rewrite by
tests/golden/make_golden_nn_plan.py; every row is recomputed here, by the generator's own probing code, on the library
under test and compared exactly: workspace sizes, every bit of mpc_mlp_supported (by widths alone and for a complete
description), the weight gradient's workspace, and the code and text with which each entry point refuses a description
before any launch.  No call here reaches a launch."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN
from mpc import _native

_spec = importlib.util.spec_from_file_location("make_golden_nn_plan", os.path.join(GOLDEN, "make_golden_nn_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "nn_plan_answers.json")) as fh:
        t = json.load(fh)
    assert tuple(t["grad_N"]) == gen.GRAD_N and tuple(t["entries"]) == gen.ENTRIES
    return gen.unpack(t)


def test_the_table_covers_what_the_generator_describes(table):
    assert [(r["n_layers"], r["widths"]) for r in table] == [(L, w) for L, w in gen.descriptions()]
    by = {tuple(r["widths"]): r for r in table}
    # one network on each side of every rule, as the library answered before the rewrite
    # (each bit is one kernel's budget: these two fit the rollout's staging and not the Jacobian's product buffers, the third neither)
    assert by[(40, 1024, 32)]["supported_by_widths"] == 1 and by[(40, 512, 512, 32)]["supported_by_widths"] == 1
    assert by[(5, 2048, 4)]["supported_by_widths"] == 0 and by[(40, 100, 32)]["supported_by_widths"] == 3
    assert by[(16, 128, 12)]["supported_by_widths"] == 3 and by[(16, 129, 12)]["supported_by_widths"] == 3
    assert by[(16, 256, 100, 12)]["workspace_bytes"] == 145920 + 256
    grad = lambda w: by[w]["complete"][0][2] & 4          # sigmoid, no ctrl_carry
    assert grad((16, 100, 12)) and grad((40, 100, 32)) and not grad((16, 256, 100, 12))


def test_every_answer_is_the_recorded_one(table):
    L = _native.load()
    for want in table:
        got = gen.answers(_native, L, want["n_layers"], want["widths"])
        for key in ("workspace_bytes", "supported_by_widths", "complete"):
            assert got[key] == want[key], (want["widths"], key, got[key], want[key])
        assert got["refusals"].keys() == want["refusals"].keys()
        for variant, calls in want["refusals"].items():
            for entry, g, w in zip(gen.ENTRIES, got["refusals"][variant], calls):
                assert g == w, (want["widths"], variant, entry, g, w)
