"""CPU-only: `MPC.forward` takes the route it took before the choice of loop was gathered into `MPC._route`
(docs/history/r26.md).

tests/golden/solve_route_expect.json was recorded by tests/golden/make_golden_solve_route.py from the commit before that change:
for every case of the generator's table, which `_iterate_*` loop `forward` ENTERED, on what dynamics, the `impl=` keyword of
its first plan, whether the ending was shared, what the ending linearised with and the exception it raised, if any.  Here
1. `MPC.solve_route` answers every row as recorded, without running anything;
2. `forward`, watched by the generator's own `observe`, does what was recorded, row by row, exactly;
3. `forward` decides once: `_route` runs once per solve, and `solve_route` makes no plan and enters no loop."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN
from mpc import _native, mpc


def _generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


gen = _generator("make_golden_solve_route")


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "solve_route_expect.json")) as fh:
        return json.load(fh)["rows"]


@pytest.fixture(scope="module")
def runs():
    """Every case once: [(what solve_route said or the exception's type, what `observe` saw, how often `_route` ran in forward)]."""
    _native.load()
    out = []
    for c in gen.cases():
        be, ctrl, args = gen.build(c)
        with gen.installed(be, c["widths"]):
            try:
                asked = ctrl.solve_route(*args)
            except Exception as e:
                asked = type(e).__name__
        assert not be.calls, (c["id"], be.calls)                 # the query ran nothing
        be, ctrl, args = gen.build(c)
        routed, inner = [], ctrl._route
        ctrl._route = lambda *a, **k: (routed.append(1), inner(*a, **k))[1]
        out.append((asked, gen.observe(c, (be, ctrl, args)), len(routed)))
    return out


def test_the_table_is_the_generators_and_covers_every_loop_flag_and_backend(table):
    assert [row["id"] for row in table] == [c["id"] for c in gen.cases()]
    assert {row["loop"] for row in table} == set(gen.LOOPS)
    assert {row["dynamics"] for row in table} == {None, "lin", "EnvSpec", "EnvSpec:carry", "MlpSpec", "MlpSpec:carry"}
    assert {row["plan"] for row in table} == {None, "auto", _native.IMPL_MFMA40_NARROW, _native.IMPL_WAVE1_CARRY}
    assert {row["shared"] for row in table} == {None, False, True}
    for flag in gen.FLAGS:
        assert any(flag in row["id"] for row in table), flag
    for backend in gen.BACKENDS:
        assert any(row["id"].startswith(backend + "|") for row in table), backend
    # a few rows as the commit before answered them
    by = {row["id"]: row for row in table}
    assert by["oracle|full|lin|gamma=None|ANALYTIC|T=1|B=3|3/2|-|widths=any"]["loop"] == "planned"
    assert by["oracle|full|pendulum|gamma=None|FINITE_DIFF|T=5|B=3|3/1|-|widths=any"]["loop"] == "general"
    assert by["oracle|full|pendulum|gamma=0.5|AUTO_DIFF|T=5|B=3|3/1|-|widths=any"]["loop"] == "general"
    assert by["carrying|full|pendulum|gamma=0.5|AUTO_DIFF|T=5|B=3|3/1|-|widths=any"]["dynamics"] == "EnvSpec:carry"
    assert by["noplans|full|nn_relu|gamma=None|ANALYTIC|T=5|B=3|3/2|-|widths=any"]["loop"] == "general"
    assert by["oracle|full|nn_relu|gamma=None|ANALYTIC|T=5|B=3|3/2|-|widths=library"]["loop"] == "general"
    assert by["hip|full|pendulum|gamma=0.5|ANALYTIC|T=5|B=3|3/1|row_carry_kernel|widths=any"]["plan"] == _native.IMPL_WAVE1_CARRY


def test_solve_route_answers_every_row_as_recorded(table, runs):
    bad = []
    for want, (asked, _, _) in zip(table, runs):
        if isinstance(asked, str):
            # the query raised: so did the solve, the same exception, before it entered a loop
            ok = want["loop"] is None and want["raises"] == asked
        else:
            assert isinstance(asked, mpc.SolveRoute) and asked._fields == ("loop", "dynamics", "ref_norm", "shared_ending")
            ok = (asked.loop, gen.kind(asked.dynamics)) == (want["loop"], want["dynamics"])
            ok = ok and asked.ref_norm == ("reference_du_norm" in want["id"] and "|B=3|" in want["id"])
            # (the ending is reached by the solves that do not raise: there `shared` is what the final step was handed)
            ok = ok and (want["shared"] is None or asked.shared_ending == want["shared"])
        if not ok:
            bad.append((want, asked))
    assert not bad, "%d rows differ, the first: %r" % (len(bad), bad[0])


def test_forward_does_what_was_recorded(table, runs):
    bad = [(want, got) for want, (_, got, _) in zip(table, runs) if got != want]
    assert not bad, "%d rows differ, the first: recorded %r, here %r" % (len(bad), bad[0][0], bad[0][1])


def test_forward_decides_once(table, runs):
    for want, (_, _, routed) in zip(table, runs):
        assert routed == 1 or (want["loop"] is None and routed <= 1), (want["id"], routed)
