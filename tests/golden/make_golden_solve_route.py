"""Which loop `MPC.forward` enters, on what dynamics, with which forced kernel, and how its differentiable ending runs -- for a table
of solves on CPU stand-in backends.

The table (solve_route_expect.json) is recorded from the commit BEFORE the routing of `MPC.forward` was gathered into one decision
(docs/history/r26.md): check that commit out, build it, then

    python tests/golden/make_golden_solve_route.py

Nothing here asks the code under test what it WOULD do: `observe` runs `forward` and watches, through wrappers on the instance,
which of `_iterate_planned` / `_iterate_slew` / `_iterate_network` / `_iterate_general` is entered first and with what dynamics
argument, the `impl=` keyword of the first `plan_step` / `plan_network_iteration`, whether the final no-op step is handed the
batch-shared arguments, what the ending linearises with, and the type of the exception where the solve raises one (a module cost
without `grad_input`, an elu network under ANALYTIC, ...: such rows stay, an exception is part of the behaviour).
tests/test_solve_route.py runs `observe` again on the code under test and compares exactly; it also holds `MPC.solve_route` to
the table.  Only names that commit already has are used here.

Cases (`cases()`): n_state / n_ctrl = 3 / 2 (the pendulum: its own 3 / 1), T = 5, B = 3, float32, one iLQR iteration.
  cost     full: QuadCost C [T,B,n,n]; shared: QuadCost C [n,n], c [n] (and a LinDx F [ns,n], f [ns]); module: an nn.Module
  dx       lin, pendulum, nn_sigmoid / nn_relu / nn_elu (NNDynamics, one hidden layer of 4), callable (a plain function)
  gamma    slew_rate_penalty None or 0.5
  grad     ANALYTIC, AUTO_DIFF, FINITE_DIFF
  T        1 or 5 (on the oracle stand-in)
  ref      reference_du_norm with B = 1 or 3
  flag     each opt-in constructor flag alone; a few rows at the sizes where `narrow_step_kernel` fires (13/4, 12/4 with a penalty)
Backends: `oracle` (tests/oracle_backend.py as it is), `carrying` (says its lane-per-problem kernel carries the control),
`noplans` (no `plan_network_iteration`), `hip` (the stand-in with `impl_supported` / `row_carry_pays` answered by the library
itself: host calls that need no device).  `MlpSpec.supported` refuses a host tensor before it looks at a network, so it is
answered True here (tests/test_nn_slew_planned.py's `any_widths`), except in the rows marked `widths=library`.
"""
import contextlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "mpc.pytorch_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch                                            # noqa: E402

from mpc import _native, mpc                            # noqa: E402
from mpc.dynamics import NNDynamics                     # noqa: E402
from mpc.env_dx import pendulum                         # noqa: E402
from mpc.mpc import GradMethods, LinDx, QuadCost        # noqa: E402
from oracle_backend import OracleBackend                # noqa: E402

OUT = os.path.join(HERE, "solve_route_expect.json")
FLAGS = ("narrow_step_kernel", "narrow_kkt_kernel", "row_carry_kernel", "shared_grad_kernel", "weight_grad_kernel",
         "planned_network_slew", "reference_du_norm")
COSTS = ("full", "shared", "module")
DXS = ("lin", "pendulum", "nn_sigmoid", "nn_relu", "nn_elu", "callable")
GRADS = ("ANALYTIC", "AUTO_DIFF", "FINITE_DIFF")
LOOPS = ("planned", "slew", "network", "general")


# ---------------------------------------------------------------------------------------------
# the stand-in backends
# ---------------------------------------------------------------------------------------------
class _CarrySteps(OracleBackend):
    """The oracle models no control carry: a simulator or a network behind the carry is answered with the nominal it was given
    (tests/test_row_carry_host.py's spy) -- the loop runs, which is all a route table needs."""

    def env_traj_cost(self, x_init, u, env, C=None, c=None, want_x=True):
        if not env.carry:
            return super().env_traj_cost(x_init, u, env, C, c, want_x)
        return x_init.unsqueeze(0).expand(u.shape[0], -1, -1).contiguous(), None

    def mlp_traj_cost(self, x_init, u, net, C=None, c=None):
        if not net.ctrl_carry:
            return super().mlp_traj_cost(x_init, u, net, C, c)
        return x_init.unsqueeze(0).expand(u.shape[0], -1, -1).contiguous(), None

    @staticmethod
    def _echo(B, like, out_x, out_u, cur_x, cur_u):
        out_x.copy_(cur_x); out_u.copy_(cur_u)
        z = torch.zeros(B, dtype=like.dtype)
        return dict(new_x=out_x, new_u=out_u, costs=z, old_costs=z, full_du_norm=z, alpha_du_norm=z, alphas=z + 1,
                    qp_iters=torch.zeros(B, dtype=torch.int32), status=torch.zeros(B, dtype=torch.int32))

    def plan_step(self, x_init, C, c, F, f, cur_x, cur_u, opts, out_x=None, out_u=None, **kw):
        if opts.true_dynamics is None or not opts.true_dynamics.carry:
            return super().plan_step(x_init, C, c, F, f, cur_x, cur_u, opts, out_x=out_x, out_u=out_u, **kw)
        return lambda: self._echo(x_init.shape[0], C, out_x, out_u, cur_x, cur_u)

    def plan_network_iteration(self, x_init, C, c, net, opts, nominals, scratch=None, impl=0):
        if not net.ctrl_carry:
            return super().plan_network_iteration(x_init, C, c, net, opts, nominals, scratch)
        outs = tuple(dict(new_x=nominals[1 - j][0], new_u=nominals[1 - j][1]) for j in (0, 1))

        def run(j, stream=None):
            outs[j].update(self._echo(x_init.shape[0], C, nominals[1 - j][0], nominals[1 - j][1], *nominals[j]))
            return outs[j]
        return run, outs, lambda: None


class Carrying(_CarrySteps):
    """tests/test_slew_planned.py's stand-in of that name: the lane-per-problem kernel carries the control of a 3-state simulator."""

    def impl_supported(self, ns, nc, dtype, impl, opts=None):
        return bool(impl == _native.IMPL_TINY and ns == 4 and opts is not None and opts.true_dynamics is not None
                    and opts.true_dynamics.carry)


class NoPlans(OracleBackend):
    """tests/test_nn_slew_planned.py's stand-in of that name, able to solve: no pre-bound network iterations."""

    @property
    def plan_network_iteration(self):
        raise AttributeError("plan_network_iteration")


class HipQueries(_CarrySteps):
    """`impl_supported` and `row_carry_pays` as the library answers them (host calls: sizes, dtype and options only)."""

    def impl_supported(self, ns, nc, dtype, impl, opts=None):
        return _native.HipBackend.impl_supported(None, ns, nc, dtype, impl, opts)

    def row_carry_pays(self, ns, nc, dtype, T, B, opts, like=None):
        return _native.HipBackend.row_carry_pays(None, ns, nc, dtype, T, B, opts, like=like)


BACKENDS = {"oracle": OracleBackend, "carrying": Carrying, "noplans": NoPlans, "hip": HipQueries}


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def case(cost="full", dx="lin", gamma=None, grad="ANALYTIC", T=5, B=3, backend="oracle", flags=(), widths="any", sizes=None):
    c = dict(cost=cost, dx=dx, gamma=gamma, grad=grad, T=T, B=B, backend=backend, flags=list(flags), widths=widths,
             sizes=list(sizes or ((3, 1) if dx == "pendulum" else (3, 2))))
    c["id"] = "%s|%s|%s|gamma=%s|%s|T=%d|B=%d|%d/%d|%s|widths=%s" % (
        backend, cost, dx, gamma, grad, T, B, c["sizes"][0], c["sizes"][1], "+".join(flags) or "-", widths)
    return c


def cases():
    out = []
    for cost, dx, gamma, grad in itertools.product(COSTS, DXS, (None, 0.5), GRADS):
        for T in (1, 5):
            out.append(case(cost, dx, gamma, grad, T))
        for backend in ("carrying", "noplans", "hip"):
            out.append(case(cost, dx, gamma, grad, backend=backend))
    for cost, dx, gamma, B in itertools.product(COSTS, DXS, (None, 0.5), (1, 3)):
        out.append(case(cost, dx, gamma, B=B, flags=("reference_du_norm",)))
    for flag, cost, dx, gamma in itertools.product(FLAGS[:-1], COSTS[:2], DXS, (None, 0.5)):
        out.append(case(cost, dx, gamma, backend="hip", flags=(flag,)))
    # the sizes at which `narrow_step_kernel` binds a kernel: 13 to 16 states at the loop's own sizes
    for flags in ((), ("narrow_step_kernel",), ("narrow_kkt_kernel",)):
        out.append(case(dx="lin", backend="hip", flags=flags, sizes=(13, 4)))
        out.append(case(dx="lin", gamma=0.5, backend="hip", flags=flags, sizes=(12, 4)))
        out.append(case(dx="nn_sigmoid", backend="hip", flags=flags, sizes=(13, 4)))
        out.append(case(dx="nn_sigmoid", gamma=0.5, backend="hip", flags=flags + ("planned_network_slew",), sizes=(12, 4)))
    for dx in DXS[2:5]:
        out.append(case(dx=dx, widths="library"))
        out.append(case(dx=dx, gamma=0.5, widths="library", flags=("planned_network_slew",)))
    assert len({c["id"] for c in out}) == len(out)
    return out


class ModuleCost(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(n))

    def forward(self, tau):
        return 0.5 * (tau * tau * self.w).sum(1) + 0.1 * tau.sum(1)


def build(c):
    """-> (backend, controller, (x_init, cost, dx)) of one case; x_init asks for a gradient, so every solve has its ending."""
    torch.manual_seed(7)
    (ns, nc), T, B = c["sizes"], c["T"], c["B"]
    n = ns + nc
    rn = lambda *s: torch.randn(*s)
    if c["cost"] == "module":
        cost = ModuleCost(n)
    elif c["cost"] == "shared":
        cost = QuadCost(torch.eye(n) + 0.1 * torch.ones(n, n), 0.1 * rn(n))
    else:
        L = rn(T, B, n, n)
        cost = QuadCost(L @ L.transpose(2, 3) / n + torch.eye(n), 0.1 * rn(T, B, n))
    A = torch.cat((torch.eye(ns), torch.zeros(ns, nc)), 1)
    if c["dx"] == "lin":
        if c["cost"] == "shared":
            dx = LinDx(A + 0.1 * rn(ns, n), 0.1 * rn(ns))
        else:
            dx = LinDx(A + 0.1 * rn(T - 1, B, ns, n), 0.1 * rn(T - 1, B, ns))
    elif c["dx"] == "pendulum":
        dx = pendulum.PendulumDx()
    elif c["dx"] == "callable":
        M = A + 0.1 * rn(ns, n)
        dx = lambda x, u: torch.cat((x, u), 1) @ M.t()
    else:
        dx = NNDynamics(ns, nc, [4], activation=c["dx"][3:])
    if c["dx"] == "pendulum":
        th = torch.linspace(-0.8, 0.8, B)
        x0 = torch.stack((th.cos(), th.sin(), 0.2 * th), 1)
    else:
        x0 = rn(B, ns)
    ctrl = mpc.MPC(ns, nc, T, lqr_iter=1, verbose=-1, exit_unconverged=False, detach_unconverged=False, n_batch=B,
                   grad_method=GradMethods[c["grad"]], slew_rate_penalty=c["gamma"], **{flag: True for flag in c["flags"]})
    return BACKENDS[c["backend"]](), ctrl, (x0.requires_grad_(True), cost, dx)


def kind(dynamics):
    """How the table names what a loop runs on."""
    if dynamics is None or isinstance(dynamics, str):
        return dynamics
    if isinstance(dynamics, _native.EnvSpec):
        return "EnvSpec:carry" if dynamics.carry else "EnvSpec"
    if isinstance(dynamics, _native.MlpSpec):
        return "MlpSpec:carry" if dynamics.ctrl_carry else "MlpSpec"
    return type(dynamics).__name__


@contextlib.contextmanager
def installed(be, widths):
    prev = _native.set_backend_for_testing(be)
    supported = _native.MlpSpec.__dict__["supported"]
    if widths == "any":
        _native.MlpSpec.supported = staticmethod(lambda weights, activation, like, bits=3: True)
    try:
        yield
    finally:
        _native.MlpSpec.supported = supported
        _native.set_backend_for_testing(prev)


def observe(c, built=None):
    """Run the solve of one case and report what it did, see the module docstring."""
    be, ctrl, args = built or build(c)
    entered, plans, ending, seen = [], [], [], {"phase": "loop", "shared": None}

    def loop(name):
        inner = getattr(ctrl, "_iterate_" + name)

        def run(*a, **k):
            # (the sixth argument -- planned: the simulator, None = the LinDx; slew, network: the plan / the spec; general has none)
            dyn = None if name == "general" else kind(a[5])
            entered.append((name, "lin" if name == "planned" and dyn is None else dyn))
            top = len(entered) == 1
            out = inner(*a, **k)
            if top:
                seen["phase"] = "ending"
            return out
        return run
    for name in LOOPS:
        setattr(ctrl, "_iterate_" + name, loop(name))

    def planner(name):
        inner = getattr(be, name)

        def run(*a, **k):
            plans.append(k["impl"] if "impl" in k else "auto")
            return inner(*a, **k)
        return run
    for name in ("plan_step", "plan_network_iteration"):
        if hasattr(be, name):
            setattr(be, name, planner(name))

    def watch(obj, name, label, when=lambda a, k: True):
        if not hasattr(obj, name):
            return
        inner = getattr(obj, name)

        def run(*a, **k):
            if seen["phase"] == "ending" and when(a, k):
                ending.append(label)
            return inner(*a, **k)
        setattr(obj, name, run)
    watch(be, "env_linearize", "env_linearize")
    watch(ctrl, "linearize_dynamics", "linearize_dynamics")
    watch(ctrl, "approximate_cost", "approximate_cost")
    step = ctrl.solve_lqr_subproblem

    def final(*a, **k):
        if k.get("no_op_forward"):
            seen["shared"] = bool(k.get("shared_grad_kernel", False))
        return step(*a, **k)
    ctrl.solve_lqr_subproblem = final
    raised = None
    with installed(be, c["widths"]):
        try:
            ctrl(*args)
        except Exception as e:          # (part of the behaviour: the type is recorded)
            raised = type(e).__name__
    return {"id": c["id"], "loop": entered[0][0] if entered else None, "dynamics": entered[0][1] if entered else None,
            "plan": plans[0] if plans else None, "shared": seen["shared"], "ending": ">".join(ending) or None, "raises": raised}


def main():
    _native.load()
    rows = [observe(c) for c in cases()]
    with open(OUT, "w") as fh:
        fh.write('{"rows": [\n')
        fh.write(",\n".join("  " + json.dumps(row, separators=(",", ":")) for row in rows))
        fh.write("\n ]}\n")
    by = {}
    for row in rows:
        by[row["loop"]] = by.get(row["loop"], 0) + 1
    print("%s: %d rows, %d bytes; loops %s; forced plans %d; raising rows %d" % (
        OUT, len(rows), os.path.getsize(OUT), by, sum(isinstance(r["plan"], int) and r["plan"] != 0 for r in rows),
        sum(r["raises"] is not None for r in rows)))


if __name__ == "__main__":
    main()
