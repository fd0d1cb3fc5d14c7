"""`MPC` -- the differentiable box-constrained iLQR driver, MI355X build.

API mirror of the reference's mpc/mpc.py (`MPC`, `QuadCost`, `LinDx`, `GradMethods`): same
constructor keywords, same `(x, u, costs)` return, same convergence / best-iterate rules
(mpc/mpc.py:245-337).  The per-iteration work is the `mpc_lqr_step` kernel; the bookkeeping the
reference does with a Python loop over the batch (best-iterate copy, `max(full_du_norm)`,
mpc/mpc.py:279-285, 299) is the `mpc_select_best` kernel, so one iLQR iteration costs two launches
and ONE small device->host read.
"""
import collections
from collections import namedtuple
from enum import Enum

import torch
from torch.nn import Module

from . import _native, util
from ._native import StepOptions
from .lqr_step import LQRStep

QuadCost = namedtuple("QuadCost", "C c")
LinDx = namedtuple("LinDx", "F f")
QuadCost.__new__.__defaults__ = (None,) * len(QuadCost._fields)
LinDx.__new__.__defaults__ = (None,) * len(LinDx._fields)
# What `MPC._route` decides, once per solve (`MPC.solve_route`).  loop: "planned", "slew", "network" or "general"; dynamics: what
# that loop runs on -- None (general), "lin", an EnvSpec or an MlpSpec; ref_norm: `reference_du_norm` with a batch
SolveRoute = namedtuple("SolveRoute", "loop dynamics ref_norm shared_ending")


class GradMethods(Enum):
    AUTO_DIFF = 1
    FINITE_DIFF = 2
    ANALYTIC = 3
    ANALYTIC_CHECK = 4


def _grad_tensors(module):
    """The tensors of a module that ask for a gradient: parameters and plain tensor attributes (the shipped simulators keep
    `params` as one), lists and tuples of them included, recursively over sub-modules."""
    for m in module.modules():
        for v in list(m.parameters(recurse=False)) + list(vars(m).values()):
            for t in (v if isinstance(v, (list, tuple)) else (v,)):
                if torch.is_tensor(t) and t.requires_grad:
                    yield t


def _any_requires_grad(obj):
    """Does a QuadCost / LinDx / module (searched by `_grad_tensors`) carry a tensor that asks for a gradient?"""
    if isinstance(obj, (QuadCost, LinDx)):
        return any(torch.is_tensor(t) and t.requires_grad for t in obj)
    return isinstance(obj, Module) and any(True for _ in _grad_tensors(obj))


def _only_params_require_grad(dx):
    """Is `dx.params` the one tensor of the module (searched by `_grad_tensors`) that asks for a gradient?"""
    prm = getattr(dx, "params", None)
    return torch.is_tensor(prm) and prm.requires_grad and all(t is prm for t in _grad_tensors(dx))


_PINNED = collections.OrderedDict()     # (device, stream, host thread) -> [pinned block, its int32 view, tag counter]; LRU, see _FlagReader
_PINNED_MAX = 64                         # a thread-per-request server would otherwise page-lock a block per thread for ever


class _FlagReader:
    """The two words the driver needs from the device per iteration (any problem improved, max ||du||).
    With the HIP backend the select kernel stores them in page-locked host memory itself, followed by a tag; `wait()` polls
    that tag -- no device-to-host copy and no event (an event's system-scope release held the next kernel back by 6 us per
    iteration).  Other backends (the test stand-ins): an asynchronous copy and an event."""

    _POLL_S = 0.005

    def __init__(self, device, dtype, be=None):
        # int32 flag at byte 0, the tag at byte 4, the maximum (float32 / float64) at byte 8 of one block
        self.cuda = device.type == "cuda"
        self._host_device = device
        self.direct = self.cuda and getattr(be, "writes_host_flags", False)
        if self.direct:
            self.device_flags = be.select_flags(device, dtype)
        else:
            self._dev = torch.empty(16, dtype=torch.uint8, device=device)
            self.device_flags = (self._dev[0:4].view(torch.int32), self._dev[8:8 + torch.empty(0, dtype=dtype).element_size()].view(dtype))
        if self.cuda:
            # page-locking memory costs milliseconds: one block per device, stream AND host thread, kept for the life of the
            # process (two solves on one stream from two threads would otherwise overwrite each other's tag and result words:
            # ADVICE r03; within a thread solves are sequential, the tag counter tells their select calls apart)
            import threading
            key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream, threading.get_ident())
            slot = _PINNED.get(key)
            if slot is None:
                blk = torch.zeros(16, dtype=torch.uint8).pin_memory()
                slot = _PINNED[key] = [blk, blk.numpy().view("int32"), 0]
                while len(_PINNED) > _PINNED_MAX:          # least recently used out; a reader still holding its slot keeps it alive
                    _PINNED.popitem(last=False)
            else:
                _PINNED.move_to_end(key)
            self._slot = slot
            self._host = self._slot[0]
            self.host = (self._host[0:4].view(torch.int32), self._host[8:8 + self.device_flags[1].element_size()].view(dtype))
            if not self.direct:
                self.event = torch.cuda.Event()

    def select_kw(self):
        """keyword arguments of the select call this reader will wait for"""
        if not self.direct:
            return {}
        self._slot[2] = (self._slot[2] % 0x7fffffff) + 1          # a tag no earlier call on this block has used (never 0)
        return dict(host=self._host, tag=self._slot[2])

    def start(self):
        if self.cuda and not self.direct:
            self._host.copy_(self._dev, non_blocking=True)
            self.event.record()

    def wait(self):
        """-> (flag bits: 1 = some problem improved, 2 = some C is not symmetric; max ||du||)"""
        if self.direct:
            words, tag = self._slot[1], self._slot[2]
            if words[1] != tag:
                import time
                t0 = time.monotonic()
                while words[1] != tag:
                    if time.monotonic() - t0 > self._POLL_S:
                        # not there after a few milliseconds: a long queue in front of the select kernel, or host memory
                        # the device's stores reach only when the kernel retires -- wait for the stream (which also
                        # surfaces a launch failure as the error it is); the words are there afterwards or never
                        torch.cuda.current_stream(self._host_device).synchronize()
                        if words[1] != tag:
                            raise RuntimeError("mpc_select_best did not report (tag %d, host word %d)" % (tag, int(words[1])))
            return int(self.host[0][0]), float(self.host[1][0])
        if self.cuda:
            self.event.synchronize()
            return int(self.host[0][0]), float(self.host[1][0])
        return int(self.device_flags[0][0]), float(self.device_flags[1][0])


class SlewRateCost(Module):
    """A module cost plus the slew-rate quadratic on the augmented variable (u_prev, x, u)
    (reference mpc/mpc.py:36-56)."""

    def __init__(self, cost, slew_C, n_state, n_ctrl):
        super().__init__()
        self.cost, self.slew_C = cost, slew_C
        self.n_state, self.n_ctrl = n_state, n_ctrl

    def forward(self, tau):
        return self.cost(tau[:, self.n_ctrl:]) + 0.5 * util.bquad(tau, self.slew_C[0])   # time-invariant

    def grad_input(self, x, u):
        raise NotImplementedError("Implement grad_input")


class UnconvergedError(AssertionError):
    """Raised where the reference does a bare `assert False` (mpc/mpc.py:321-324): some problem did
    not reach a fixed point and exit_unconverged=True."""


class MPC(Module):
    """A differentiable box-constrained iLQR solver.

        min_{tau={x,u}} sum_t 0.5 tau_t^T C_t tau_t + c_t^T tau_t
                        s.t. x_{t+1} = f(x_t, u_t),  x_0 = x_init,  u_lower <= u <= u_upper

    Constructor arguments are those of the reference (mpc/mpc.py:123-144): n_state, n_ctrl, T,
    u_lower/u_upper (floats or [T,B,n_ctrl]), u_zero_I, u_init, lqr_iter, grad_method, delta_u,
    verbose, eps, back_eps, n_batch, linesearch_decay, max_linesearch_iter, exit_unconverged,
    detach_unconverged, backprop, slew_rate_penalty, prev_ctrl, not_improved_lim, best_cost_eps.
    """

    def __init__(self, n_state, n_ctrl, T, u_lower=None, u_upper=None, u_zero_I=None, u_init=None,
                 lqr_iter=10, grad_method=GradMethods.ANALYTIC, delta_u=None, verbose=0, eps=1e-7,
                 back_eps=1e-7, n_batch=None, linesearch_decay=0.2, max_linesearch_iter=10,
                 exit_unconverged=True, detach_unconverged=True, backprop=True, slew_rate_penalty=None,
                 prev_ctrl=None, not_improved_lim=5, best_cost_eps=1e-4, reference_du_norm=False,
                 narrow_step_kernel=False, narrow_kkt_kernel=False, row_carry_kernel=False, shared_grad_kernel=False,
                 f64_grad_kernel=False, f64_weight_grad_kernel=False, weight_grad_kernel=False, planned_network_slew=False):
        super().__init__()
        assert (u_lower is None) == (u_upper is None)
        assert max_linesearch_iter > 0
        self.n_state, self.n_ctrl, self.T = n_state, n_ctrl, T
        self.u_lower = u_lower if isinstance(u_lower, float) else util.detach_maybe(u_lower)
        self.u_upper = u_upper if isinstance(u_upper, float) else util.detach_maybe(u_upper)
        self.u_zero_I = util.detach_maybe(u_zero_I)
        self.u_init = util.detach_maybe(u_init)
        self.lqr_iter = lqr_iter
        self.grad_method = grad_method
        self.delta_u = delta_u
        self.verbose = verbose
        self.eps = eps
        self.back_eps = back_eps
        self.n_batch = n_batch
        self.linesearch_decay = linesearch_decay
        self.max_linesearch_iter = max_linesearch_iter
        self.exit_unconverged = exit_unconverged
        self.detach_unconverged = detach_unconverged
        self.backprop = backprop
        self.not_improved_lim = not_improved_lim
        self.best_cost_eps = best_cost_eps
        self.slew_rate_penalty = slew_rate_penalty
        # (not in the reference) True: `full_du_norm` as the reference computes it for n_batch > 1 -- a transpose in front of the
        # reshape mixes the problems of a batch (mpc/lqr_step.py:243-245) -- so that the eps exit (:299) and the detach mask
        # (:321-334) are the reference's.  Default: each problem's own norm.  Costs one more rollout per iteration
        # and takes the general loop (no pre-bound device-side iterations).
        self.reference_du_norm = bool(reference_du_norm)
        # OPT-IN: the differentiable linearisation of a trainable NNDynamics as _native.MlpLinearizeFn (mpc_mlp_linearize forward,
        # mpc_mlp_param_grad backward) instead of the module through torch autograd.  Off by default: measured faster than the
        # module route at (12, 4, [100]) but slower at (32, 8, [100]) (docs/history/r10.md)
        self.weight_grad_kernel = bool(weight_grad_kernel)
        # OPT-IN: the same for a float64 NNDynamics (mpc_mlp_linearize_dtype forward, mpc_mlp_param_grad_dtype backward, both MPC_F64).
        # `weight_grad_kernel` keeps governing float32 only; off by default (docs/history/r32.md)
        self.f64_weight_grad_kernel = bool(f64_weight_grad_kernel)
        # OPT-IN: a slew-rate penalty around an NNDynamics on the pre-bound device loop (`_iterate_slew` -> `_iterate_network` on the
        # augmented problem, mpc_mlp_linearize_carry) instead of `_iterate_general` (which networks: `solve_route`).  Off by default
        # whatever it measures: tests/test_gpu_nn.py::test_slew_rate_penalty_on_the_network_kernels and tests/test_gpu_nn_wide.py::
        # test_slew_rate_penalty_on_a_wide_network pin the general route by spying on HipBackend.mlp_rollout, a method a pre-bound
        # iteration never goes through (it calls mpc_mlp_rollout itself), and existing tests are the yardstick of every change
        self.planned_network_slew = bool(planned_network_slew)
        # OPT-IN: the pre-bound loops (`_iterate_planned`, through it `_iterate_slew`, and `_iterate_network`) bind their step plans
        # with _native.IMPL_MFMA40_NARROW -- the padded 32/8 kernel on one 16-row state tile -- instead of IMPL_AUTO, where
        # `_forced_impl` says so at the sizes the loop runs at (n_state + n_ctrl states on the slew route: 12/4 becomes 16/4) --
        # shapes up to 12/4 have faster kernels of their own and stay auto's.  Everywhere else IMPL_AUTO, as ever.
        # A forced kernel reads C through its symmetry and only FLAGS a C that is not symmetric, where impl 0 solves such a
        # problem again: a narrow-bound loop whose first step reports the bit starts over on IMPL_AUTO plans (`_drive`), so x, u
        # and costs are the flag-off solve's for every C.  The price: iteration 1 is launched after the flags of iteration 0 are
        # in, not before.
        # Off by default: the kernel auto picks for these shapes is pinned by existing tests
        # (tests/golden/step_route_expect.json, tests/test_gpu_step_route.py), which are the yardstick of every change, and the
        # narrow kernel's time against the padded one is a measurement of docs/history/r16.md, not a promise.  The
        # differentiable ending and the KKT backward do not look at the flag
        self.narrow_step_kernel = bool(narrow_step_kernel)
        # OPT-IN: the differentiable ending's backward asks for the one-state-tile fused KKT kernels (LQRStep(narrow_kkt_kernel=True):
        # _native.KKT_PREFER_NARROW -- 13 to 16 states, float32, C symmetric; every other backward is routed as without it).  With a
        # slew_rate_penalty (12/4 differentiates at 16/4) the ending then also makes the symmetry promise the plain ending makes --
        # `_c_symmetric`, which the slew loop established on the AUGMENTED C, and `_slew_compose` adds symmetric blocks only -- so
        # that its backward is the fused one at all; flag off it makes none and takes the three-call route, as ever.  Where the
        # loop's first step flagged a C that is not symmetric no promise is made and the gradients are the flag-off solve's.
        # Off by default: the padded kernel is what existing tests pin, the narrow one's time is docs/history/r19.md's measurement
        self.narrow_kkt_kernel = bool(narrow_kkt_kernel)
        # OPT-IN: a slew-rate solve around a shipped simulator (`_iterate_slew` -> `_iterate_planned` with the simulator behind
        # ENV_CTRL_CARRY) binds its step plans with _native.IMPL_WAVE1_CARRY -- a 16-lane row per problem instead of a lane per
        # problem -- where `_forced_impl` says so at the sizes the loop runs at.  Everywhere else -- float64, a LinDx slew solve, a
        # larger batch, a backend without the query -- IMPL_AUTO, as ever: bitwise the flag-off solve.  Off by default: auto routes
        # every carry call to the lane-per-problem kernel and existing tests pin that; the row kernel's time against it is a
        # measurement of docs/history/r21.md, not a promise.  The differentiable ending does not look at the flag
        self.row_carry_kernel = bool(row_carry_kernel)
        # OPT-IN: a QuadCost / LinDx given in batch-shared form (C [T,n,n] or [n,n], c [T,n] or [n], F [T-1,ns,n] or [ns,n], f
        # likewise) reaches the final no-op step UN-expanded, whose backward then sums the gradients over the batch inside the
        # kernels (lqr_step._LQRStepSharedFn, mpc_lqr_kkt_grads_shared) instead of writing one [n,n] block per problem for
        # autograd's expand to add up.  The iterations are untouched.  Which solves (`solve_route`: `shared_ending`); views the
        # caller expanded themselves keep the per-problem route.  Off by default (docs/history/r14.md)
        self.shared_grad_kernel = bool(shared_grad_kernel)
        # OPT-IN: the differentiable ending's backward runs the closed-form part of a float64 problem with n_state + n_ctrl <= 64
        # (the augmented sizes on the slew ending) on the float64 wavefront kernels (LQRStep(f64_grad_kernel=True):
        # _native.KKT_GRADS_WAVE64, mpc_lqr_kkt_grads_kernel) instead of the generic kernel.  Float32 solves and larger shapes are
        # routed as without it; the iterations and the nested solve are untouched.  Off by default: mpc_lqr_kkt_grads in float64 is
        # pinned to the generic kernel by existing tests (docs/history/r27.md has the times)
        self.f64_grad_kernel = bool(f64_grad_kernel)
        self.flag_reducer = None     # set by mpc.shard for lock-step sharded solves
        self.prev_ctrl = prev_ctrl

    # ------------------------------------------------------------------------------------------
    def _expand_cost(self, cost, n_batch):
        """[n,n] / [T,n,n] costs are broadcast to [T,B,n,n] as stride-0 views (never copied: the
        kernels read them through their strides, so a shared cost matrix stays L2-resident)."""
        C, c = cost
        n = self.n_state + self.n_ctrl
        if C.ndimension() == 2:
            C = C.unsqueeze(0).unsqueeze(0).expand(self.T, n_batch, n, n)
        elif C.ndimension() == 3:
            C = C.unsqueeze(1).expand(self.T, n_batch, n, n)
        if c.ndimension() == 1:
            c = c.unsqueeze(0).unsqueeze(0).expand(self.T, n_batch, n)
        elif c.ndimension() == 2:
            c = c.unsqueeze(1).expand(self.T, n_batch, n)
        if C.ndimension() != 4 or c.ndimension() != 3:
            raise ValueError("MPC Error: Unexpected QuadCost shape.")
        return QuadCost(C, c)

    def _expand_dx(self, dx, n_batch):
        """[ns,n] / [T-1,ns,n] linear models (f [ns] / [T-1,ns], or None) are broadcast to [T-1,B,ns,n] as stride-0 views,
        exactly like the cost."""
        F, f = dx
        ns, n = self.n_state, self.n_state + self.n_ctrl
        if F.ndimension() == 2:
            F = F.unsqueeze(0).unsqueeze(0).expand(self.T - 1, n_batch, ns, n)
        elif F.ndimension() == 3:
            F = F.unsqueeze(1).expand(self.T - 1, n_batch, ns, n)
        if f is not None and f.numel() > 0:
            if f.ndimension() == 1:
                f = f.unsqueeze(0).unsqueeze(0).expand(self.T - 1, n_batch, ns)
            elif f.ndimension() == 2:
                f = f.unsqueeze(1).expand(self.T - 1, n_batch, ns)
            if f.ndimension() != 3:
                raise ValueError("MPC Error: Unexpected LinDx shape.")
        if F.ndimension() != 4:
            raise ValueError("MPC Error: Unexpected LinDx shape.")
        return LinDx(F, f)

    def _expand_args(self, x_init, cost, dx):
        """What `forward` and `solve_route` start from -> (n_batch, cost, dx), a QuadCost / LinDx as [T,B,...] views."""
        assert isinstance(cost, (QuadCost, Module)) or callable(cost)
        assert isinstance(dx, (LinDx, Module)) or callable(dx)
        if self.n_batch is not None:
            n_batch = self.n_batch
        elif isinstance(cost, QuadCost) and cost.C.ndimension() == 4:
            n_batch = cost.C.size(1)
        else:
            raise ValueError("MPC Error: Could not infer batch size, pass in as n_batch")
        if isinstance(cost, QuadCost):
            cost = self._expand_cost(cost, n_batch)
        if isinstance(dx, LinDx) and torch.is_tensor(dx.F) and dx.F.ndimension() < 4:
            dx = self._expand_dx(dx, n_batch)
        assert x_init.ndimension() == 2 and x_init.size(0) == n_batch
        return n_batch, cost, dx

    def solve_route(self, x_init, cost, dx):
        """The `SolveRoute` that `forward(x_init, cost, dx)` would take; nothing runs.  The rules, the first that holds:
        general   a module cost, or `reference_du_norm` with a batch: every pre-bound loop below needs a QuadCost and each
                  problem's own du norm.  `_iterate_general`: linearisation and cost expansion through torch, an LQRStep a turn.
        slew      a `slew_rate_penalty`, T > 1 and dynamics `_slew_plan` names: "lin" for a LinDx; the augmented EnvSpec of a
                  shipped simulator with one control under ANALYTIC / AUTO_DIFF (FINITE_DIFF keeps the reference's central
                  differences) on a backend whose lane-per-problem kernel carries the control; with `planned_network_slew` the
                  augmented MlpSpec of a network as under `network`, n_state + n_ctrl <= 32, in a dtype the backend's augmented
                  linearisation exists in (HipBackend: float32), whose rollout kernels take the augmented widths.  The loop of
                  `planned` / `network` on the augmented problem, built once (round 11).
                  Any other penalty: general.
        planned   a LinDx (any T); or T > 1 and a shipped simulator (`native_env`) under ANALYTIC / AUTO_DIFF: closed-form
                  linearisation and the simulator inside the step kernel.
        network   T > 1, ANALYTIC, a backend with `plan_network_iteration` and an NNDynamics the kernels take (`native_net`: float32
                  or float64 on the device, <= 4 layers, n_state <= 32) that is not elu (no grad_input in the reference: the
                  module refuses, mpc/dynamics.py:113-114): the whole iteration is three pre-bound C calls (round 5).
        general   everything else.
        `shared_ending`: `shared_grad_kernel` on a pre-bound loop without a penalty.  Which kernel such a loop forces
        (`narrow_step_kernel`, `row_carry_kernel`) is `_forced_impl`'s answer, at the sizes the loop runs at."""
        _, cost, dx = self._expand_args(x_init, cost, dx)
        return self._route(x_init, cost, dx, _native.backend())

    def _route(self, x_init, cost, dx, be):
        """`solve_route` on expanded arguments: the one place that chooses the loop.  Launches nothing."""
        ref_norm, penalty = self._ref_norm(x_init), self.slew_rate_penalty is not None
        prebound = isinstance(cost, QuadCost) and not ref_norm           # what every pre-bound loop needs
        loop, dynamics = "general", None
        if not prebound:
            pass
        elif penalty:
            loop, dynamics = "slew", self._slew_plan(cost, dx, be, x_init)
        elif isinstance(dx, LinDx):
            loop, dynamics = "planned", "lin"
        elif self.T > 1 and self._closed_form_env(dx):
            loop, dynamics = "planned", dx.native_env()
        elif self.T > 1:
            loop, dynamics = "network", self._kernel_net(dx, be, x_init)
        if dynamics is None:                                             # (`_slew_plan` / `_kernel_net` declined)
            loop = "general"
        return SolveRoute(loop, dynamics, ref_norm, self.shared_grad_kernel and prebound and not penalty)

    def _ref_norm(self, x_init):
        return self.reference_du_norm and x_init.size(0) > 1

    def _closed_form_env(self, dx):
        """A shipped simulator (mpc.env_dx) under a grad method for which the kernels' closed-form linearisation stands in?"""
        return hasattr(dx, "native_env") and self.grad_method in (GradMethods.ANALYTIC, GradMethods.AUTO_DIFF)

    def _kernel_net(self, dx, be, x_init):
        """The MlpSpec of an NNDynamics the pre-bound network iterations run (see `solve_route`: network), else None."""
        if self.grad_method != GradMethods.ANALYTIC or not hasattr(dx, "native_net") or not hasattr(be, "plan_network_iteration"):
            return None
        net = dx.native_net(x_init)
        return None if net is None or net.activation == "elu" else net

    def forward(self, x_init, cost, dx):
        given_cost, given_dx = cost, dx           # as the caller gave them: what `shared_grad_kernel` hands to the final step
        n_batch, cost, dx = self._expand_args(x_init, cost, dx)

        T, ns, nc = self.T, self.n_state, self.n_ctrl
        if self.u_init is None:
            u = torch.zeros(T, n_batch, nc, dtype=x_init.dtype, device=x_init.device)
        else:
            u = self.u_init
            if u.ndimension() == 2:
                u = u.unsqueeze(1).expand(T, n_batch, -1).clone()
            u = u.to(dtype=x_init.dtype, device=x_init.device)

        if self.verbose > 0:
            print("Initial mean(cost): {:.4e}".format(
                util.get_cost(T, u, cost, dx, x_init=x_init).mean().item()))

        be = _native.backend()
        route = self._route(x_init, cost, dx, be)
        if route.loop == "general":
            best = self._iterate_general(be, x_init, u, cost, dx)
        else:
            iterate = (self._iterate_planned if route.loop == "planned" else
                       self._iterate_slew if route.loop == "slew" else self._iterate_network)
            best = iterate(be, x_init, u, cost, dx, route.dynamics, n_batch)

        x, u = best["x"], best["u"]
        full_du_norm = best["full_du_norm"]
        if not self._wants_graph(x_init, cost, dx):
            # nothing upstream asks for a gradient: the differentiable re-linearisation and the no-op
            # step of mpc/mpc.py:308-319 would only build a graph nobody can reach
            self._check_converged(full_du_norm)
            return (x, u, best["costs"])
        # batch-shared arguments stay un-expanded for the final step (its Function expands them itself and returns their
        # gradients summed over the batch); everything that keeps the per-problem route gets the views as before
        shared = route.shared_ending
        if isinstance(dx, LinDx):
            F, f = (given_dx.F, given_dx.f) if shared else (dx.F, dx.f)
        elif route.loop == "planned" and not _any_requires_grad(dx):
            # a simulator whose parameters are constants here: closed-form kernel instead of autograd
            Fl, fl = be.env_linearize(route.dynamics, x[:-1].reshape(-1, ns), u[:-1].reshape(-1, nc))
            F, f = Fl.view(T - 1, n_batch, ns, ns + nc), fl.view(T - 1, n_batch, ns)
        else:
            F, f = self.linearize_dynamics(x, u, dx, diff=True)
        if isinstance(cost, QuadCost):
            C, c = (given_cost.C, given_cost.c) if shared else (cost.C, cost.c)
        else:
            C, c, _ = self.approximate_cost(x, u, cost, diff=True)

        # attach the KKT backward at the best iterate (no compute), mpc/mpc.py:318-319
        x, u = self.solve_lqr_subproblem(x_init, C, c, F, f, cost, dx, x, u, no_op_forward=True, shared_grad_kernel=shared)

        if self._check_converged(full_du_norm):
            keep = (full_du_norm < self.eps).to(x.dtype).view(1, -1, 1)
            x = x * keep + x.detach() * (1. - keep)
            u = u * keep + u.detach() * (1. - keep)
        return (x, u, best["costs"])

    def _iterate_planned(self, be, x_init, u, cost, dx, dynamics, n_batch):
        """The iLQR loop (mpc/mpc.py:245-306) when the whole iteration lives on the device: QuadCost with a LinDx
        (`dynamics` "lin") or a shipped simulator (its EnvSpec).  Inner iterations are never differentiated (the reference detaches
        them too).  Two pre-bound step plans ping-pong the nominal between two buffers, so an iteration is
        one C call (a simulator is linearised inside that call) -- no allocation, no autograd node.
        The states of a rollout ARE get_traj of its controls (:251 recomputes them).
        The convergence flags of iteration i are read back while iteration i+1 already runs: the next
        step is launched speculatively and simply not used if the flags say stop."""
        T, sim = self.T, None if dynamics == "lin" else dynamics
        xi = util.detach_maybe(x_init)
        ua = self._own_nominal(u)
        opts = self._step_options()
        if sim is not None:
            xa, _ = be.env_traj_cost(xi, ua, sim)                         # util.get_traj, :251
            # linearize_dynamics (:490-549) happens inside the step kernel: no F, f round trip through memory
            sim.linearize = True
            F = f = None
            opts.true_dynamics = sim
        else:
            xa = util.get_traj(T, ua, x_init=xi, dynamics=dx).contiguous()
            F, f = dx.F, dx.f
            # every nominal of this loop obeys (F, f) by construction: get_traj above, then each step's own rollout
            opts.nominal_on_dynamics = True
        xb, ub = torch.empty_like(xa), torch.empty_like(ua)
        # (a forced kernel rides in the plan; its variants below keep it)
        kwi, restart = self._forced_impl(be, xi, ua, sim, opts)
        variant = getattr(be, "plan_variant", None)      # (the test backends build every plan from scratch)
        # the raw stream handle, looked up once (torch.cuda.current_stream costs 4 us a call, two calls an iteration)
        stream = torch.cuda.current_stream(xa.device).cuda_stream if xa.is_cuda and variant is not None else None
        plans = [None, None]

        def bind(kw):
            """the two ping-pong plans with the impl of `kw`; iteration 0 launched in between -> its outputs"""
            plans[0] = be.plan_step(xi, cost.C, cost.c, F, f, xa, ua, opts, out_x=xb, out_u=ub, **kw)
            # the first step is on its way before anything else of the loop is set up (host time hidden)
            r0 = plans[0]() if stream is None else plans[0](stream)
            if variant is not None:
                plans[1] = variant(plans[0], cur_x=xb, cur_u=ub, out_x=xa, out_u=ua)
            else:
                plans[1] = be.plan_step(xi, cost.C, cost.c, F, f, xb, ub, opts, out_x=xa, out_u=ua, **kw)
            return r0, ((plans[0].outputs, plans[1].outputs) if variant is not None else None)
        r, outputs = bind(kwi)
        # C does not change during the solve: once the first step has reported that it is symmetric (no
        # MPC_ST_C_ASYMMETRIC in its status, read back with the convergence flags), the remaining steps run with the
        # promise MPC_OPT_C_SYMMETRIC -- no symmetry test in the kernel, no gated second launch behind it
        self._c_symmetric = False
        sym_plans = None

        def launch(i):
            plan = (sym_plans if sym_plans is not None else plans)[i % 2]
            return plan() if stream is None else plan(stream)

        def on_symmetric():
            # (a simulator solve runs on the lane-per-problem kernel, which keeps Q and V general and has no test to
            #  skip: building two more plans would only cost host time in a loop that is launch-latency bound)
            nonlocal sym_plans
            if self.lqr_iter > 2 and sim is None:
                import copy
                so = copy.copy(opts)
                so.c_symmetric = True
                if variant is not None:          # the same structs with one more option bit: no walk, no allocation
                    sym_plans = (variant(plans[0], opts=so), variant(plans[1], opts=so))
                else:
                    sym_plans = (be.plan_step(xi, cost.C, cost.c, F, f, xa, ua, so, out_x=xb, out_u=ub, **kwi),
                                 be.plan_step(xi, cost.C, cost.c, F, f, xb, ub, so, out_x=xa, out_u=ua, **kwi))
        # `restart` (see `narrow_step_kernel` in __init__): a loop whose first step reports MPC_ST_C_ASYMMETRIC starts over on IMPL_AUTO
        # plans; the nominal of iteration 0 is still in (xa, ua) -- `_drive` holds iteration 1 back until the flags are in
        return self._drive(be, launch, outputs, r, xa, ua, n_batch, stream, on_symmetric,
                           on_asymmetric=(lambda: bind({})) if restart else None)

    def _own_nominal(self, u):
        """The nominal controls of a pre-bound loop, whose iterations WRITE into them: this solve's own buffer, never the caller's
        u_init (detach / to / contiguous all return the same storage for a contiguous tensor)."""
        ua = util.detach_maybe(u).contiguous()
        if self.u_init is not None and ua.untyped_storage().data_ptr() == self.u_init.untyped_storage().data_ptr():
            ua = ua.clone()
        return ua

    def _forced_impl(self, be, xi, ua, sim, opts):
        """The kernel forced on the plans of a pre-bound loop, at the sizes it runs at -> (dict(impl=...) or {} = IMPL_AUTO as ever,
        does the loop start over on an asymmetric C).  Flag off, its predicates are not asked.  `narrow_step_kernel` first:
        IMPL_MFMA40_NARROW where the backend takes the step for it and NOT for IMPL_DPP16_PAD (up to 12/4 the 4-problems-per-wave
        kernels are auto's choice and stay it).  Where that declined, `row_carry_kernel`: IMPL_WAVE1_CARRY for a float32 simulator
        behind ENV_CTRL_CARRY where the row-per-problem carry kernel takes the step and pays at this horizon and batch; it keeps Q
        and V general like the lane-per-problem one and sets no MPC_ST_C_ASYMMETRIC: nothing to start over from."""
        if not (self.narrow_step_kernel or self.row_carry_kernel):
            return {}, False
        asks = hasattr(be, "impl_supported")
        ns, nc, T, B = int(xi.shape[1]), int(ua.shape[2]), int(ua.shape[0]), int(ua.shape[1])
        if (self.narrow_step_kernel and asks and be.impl_supported(ns, nc, xi.dtype, _native.IMPL_MFMA40_NARROW, opts)
                and not be.impl_supported(ns, nc, xi.dtype, _native.IMPL_DPP16_PAD, opts)):
            return dict(impl=_native.IMPL_MFMA40_NARROW), True
        if (self.row_carry_kernel and sim is not None and getattr(sim, "carry", False) and xi.dtype == torch.float32
                and asks and hasattr(be, "row_carry_pays") and be.impl_supported(ns, nc, xi.dtype, _native.IMPL_WAVE1_CARRY, opts)
                and be.row_carry_pays(ns, nc, xi.dtype, T, B, opts, like=xi)):
            return dict(impl=_native.IMPL_WAVE1_CARRY), False
        return {}, False

    def _slew_plan(self, cost, dx, be, x_init):
        """Does this slew-rate solve run on the device-side loop (`_iterate_slew`)?  None = no: `_iterate_general`, as before
        round 11.  Else what the dynamics are there: "lin" (LinDx), the simulator's EnvSpec behind MPC_ENV_CTRL_CARRY, or the
        augmented MlpSpec of an NNDynamics (`ctrl_carry`).  The rules: `solve_route`.  (Module costs are not augmented by the
        reference either; `MlpSpec.augmented()` does not ask the LDS budget again: mpc_mlp_supported's rollout bit does here.)"""
        if not isinstance(cost, QuadCost) or self._ref_norm(x_init) or self.slew_rate_penalty is None or self.T <= 1:
            return None
        if isinstance(dx, LinDx):
            return "lin"
        if (self._closed_form_env(dx) and self.n_ctrl == 1 and hasattr(be, "impl_supported")
                and x_init.dtype in (torch.float32, torch.float64)):
            env = dx.native_env().augmented()
            if env.n_state == self.n_state + 1 and be.impl_supported(
                    env.n_state, 1, x_init.dtype, _native.IMPL_TINY, StepOptions(true_dynamics=env)):
                return env
        # (a backend says in which dtypes its augmented-layout linearisation exists -- HipBackend: float32, so a float64 network
        # keeps the general loop, whose CtrlPassthroughDynamics rollout may still run in the kernels; a backend that says nothing
        # takes every dtype)
        if (self.planned_network_slew and self.n_state + self.n_ctrl <= 32
                and x_init.dtype in getattr(be, "carry_linearize_dtypes", (x_init.dtype,))):
            net = self._kernel_net(dx, be, x_init)
            if net is not None and net.n_state == self.n_state and net.n_ctrl == self.n_ctrl:
                aug = net.augmented()
                # (bit 0 only: the augmented network is rolled out, never linearised -- that is `net` itself, which native_net vouched for)
                if _native.MlpSpec.supported(aug.weights, aug.activation, x_init, bits=1):
                    return aug
        return None

    def _iterate_slew(self, be, x_init, u, cost, dx, plan, n_batch):
        """The loop of `_iterate_planned` on the slew-rate augmentation (mpc/mpc.py:362-445): state z_t = (u_{t-1}, x_t),
        0.5 gamma |u_t - u_{t-1}|^2 inside the stage cost.  (aC, ac, aF, af) are constant over the solve and built ONCE
        (mpc_slew_augment where the backend has it, else the torch composition); the augmented rollout of a step IS the next
        augmented nominal, so nothing is re-packed between iterations.  A simulator is carried through the kernels by
        MPC_ENV_CTRL_CARRY (its F, f never exist); an NNDynamics (`plan` = its augmented MlpSpec) runs `_iterate_network` on the
        augmented problem, whose linearisation kernel writes (aF, af) at every nominal.  `costs` include the penalty, as the
        reference's (its line search prices the augmented QuadCost); the first n_ctrl state columns are stripped from the best iterate."""
        nc = self.n_ctrl
        C, c = util.detach_maybe(cost.C), util.detach_maybe(cost.c)
        lin = isinstance(dx, LinDx)
        F, f = (util.detach_maybe(dx.F), util.detach_maybe(dx.f)) if lin else (None, None)
        if hasattr(be, "slew_augment") and C.is_cuda:
            aC, ac, aF, af = be.slew_augment(C, c, F, f, self.n_state, nc, self.slew_rate_penalty)
        else:
            _, aC, ac, aF, af = self._slew_compose(C, c, F, f)
        prev_u = self._slew_prev_u(n_batch, dict(dtype=C.dtype, device=C.device))
        ax_init = torch.cat((prev_u[0], util.detach_maybe(x_init)), 1)
        if isinstance(plan, _native.MlpSpec):
            from .dynamics import CtrlPassthroughDynamics
            # (the module serves the first get_traj only; every later nominal is a rollout of the kernels)
            best = self._iterate_network(be, ax_init, u, QuadCost(aC, ac), CtrlPassthroughDynamics(dx), plan, n_batch)
        else:
            best = self._iterate_planned(be, ax_init, u, QuadCost(aC, ac), LinDx(aF, af) if lin else None, plan, n_batch)
        best["x"] = best["x"][:, :, nc:].contiguous()
        return best

    def _drive(self, be, launch, outputs, r, xa, ua, n_batch, stream, on_symmetric, on_asymmetric=None):
        """The loop of mpc/mpc.py:245-306 around pre-bound iterations: launch(i) enqueues iteration i and returns its output
        dict (`outputs`: the two dicts the iterations alternate between, for the pre-bound select call; None = the test
        backends' general entry), `r` = the outputs of iteration 0, already on its way.  Best-iterate tracking on the device
        (:271-285); the convergence flags of iteration i are read back while iteration i+1 already runs."""
        best = dict(x=torch.empty_like(xa), u=torch.empty_like(ua),
                    costs=torch.empty(n_batch, dtype=xa.dtype, device=xa.device),
                    full_du_norm=torch.empty(n_batch, dtype=xa.dtype, device=xa.device))
        reader = _FlagReader(xa.device, xa.dtype, be)
        # (the HIP backend binds the select call's arguments once per solve; the test stand-ins take the general entry)
        def bind_select(outs_):
            if reader.direct and hasattr(be, "plan_select") and outs_ is not None:
                return be.plan_select(self.best_cost_eps, outs_, best, reader.device_flags, host=reader._host)
            return None
        sel = bind_select(outputs)
        n_not_improved, i = 0, 0
        while True:
            # best-iterate tracking, :271-285 -- on the device
            if sel is not None:
                sel(i % 2, i == 0, reader.select_kw()["tag"], i == 0, stream)
            else:
                be.select_best(i == 0, self.best_cost_eps, r["new_x"], r["new_u"], r["costs"], r["full_du_norm"],
                               best, flags=reader.device_flags, status=r["status"] if i == 0 else None, **reader.select_kw())
            reader.start()
            # `on_asymmetric` (a loop bound to a FORCED kernel): iteration 1 would overwrite the nominal iteration 0 started from,
            # which a solve that has to start over still needs -- it waits for the flags of iteration 0, this once
            hold = i == 0 and on_asymmetric is not None
            nxt = launch(i + 1) if i + 1 < self.lqr_iter and not hold else None        # overlaps the read-back
            bits, max_du_norm = reader.wait()
            if hold:
                if bits & 2:
                    # the forced kernel met a C that is not symmetric: the plans again on IMPL_AUTO, iteration 0 again
                    r, outputs = on_asymmetric()
                    sel, on_asymmetric = bind_select(outputs), None
                    on_symmetric = lambda: None          # (C is known not to be symmetric: no MPC_OPT_C_SYMMETRIC plans)
                    continue
                on_asymmetric = None
                nxt = launch(i + 1) if i + 1 < self.lqr_iter else None
            any_improved = (bits & 1) != 0
            if i == 0 and not (bits & 2):
                self._c_symmetric = True
                on_symmetric()
            if self.flag_reducer is not None:          # shards agree on the batch-wide stop test (mpc.shard)
                any_improved, max_du_norm = self.flag_reducer(any_improved, max_du_norm)
            n_not_improved += 1
            if any_improved:
                n_not_improved = 0
            if self.verbose > 0:
                util.table_log("lqr", (
                    ("iter", i),
                    ("mean(cost)", best["costs"].mean().item(), "{:.4e}"),
                    ("||full_du||_max", max_du_norm, "{:.2e}"),
                    ("mean(alphas)", float(r["alphas"].mean()), "{:.2e}"),
                    ("total_qp_iters", float(r["qp_iters"].max().item())),
                ))
            if max_du_norm < self.eps or n_not_improved > self.not_improved_lim or nxt is None:
                break
            r, i = nxt, i + 1
        return best

    def _iterate_network(self, be, x_init, u, cost, dx, net, n_batch):
        """The loop when dx is an NNDynamics the kernels take (`net` = its MlpSpec) and the cost a QuadCost: per iteration
        MPC.linearize_dynamics (mpc/mpc.py:495-512), lqr_backward and lqr_forward through the network (mpc/lqr_step.py:52-261,
        module branch :223-225) as three pre-bound C calls (HipBackend.plan_network_iteration); the states of a rollout ARE
        util.get_traj of its controls through the network (:251 recomputes them), so only the first nominal needs get_traj.
        Inner iterations are never differentiated (the reference detaches them too)."""
        T = self.T
        xi = util.detach_maybe(x_init).contiguous()
        ua = self._own_nominal(u)
        if hasattr(be, "mlp_traj_cost"):
            # util.get_traj's own call for such a module, with the spec already in hand (`dx.native_net` would build it again --
            # for the slew-rate augmentation a second set of concatenated weights)
            xa = be.mlp_traj_cost(xi, ua.to(xi.dtype), net)[0].contiguous()
        else:
            xa = util.get_traj(T, ua, x_init=xi, dynamics=dx).contiguous()
        xb, ub = torch.empty_like(xa), torch.empty_like(ua)
        nopts = self._step_options()
        kwi, restart = self._forced_impl(be, xi, ua, None, nopts)
        stream = torch.cuda.current_stream(xa.device).cuda_stream if xa.is_cuda else None
        bound = [None, None]

        def bind(kw):
            bound[0], outs_, bound[1] = be.plan_network_iteration(xi, cost.C, cost.c, net, nopts, ((xa, ua), (xb, ub)), **kw)
            return bound[0](0, stream), outs_
        r, outs = bind(kwi)
        self._c_symmetric = False

        def on_symmetric():
            if self.lqr_iter > 2:
                bound[1]()
        # (a sweep forced onto the narrow kernel that reports a non-symmetric C: the loop starts over on IMPL_AUTO, see
        # `_iterate_planned`)
        return self._drive(be, lambda i: bound[0](i % 2, stream), outs, r, xa, ua, n_batch, stream, on_symmetric,
                           on_asymmetric=(lambda: bind({})) if restart else None)

    def _iterate_general(self, be, x_init, u, cost, dx):
        """The same loop with module-valued cost / dynamics or a slew penalty: linearisation and cost
        expansion through torch, the LQR step through `solve_lqr_subproblem`."""
        T = self.T
        best = None
        n_not_improved = 0
        self._c_symmetric = False
        for i in range(self.lqr_iter):
            u = util.detach_maybe(u)
            x = util.get_traj(T, u, x_init=x_init, dynamics=dx)
            if isinstance(dx, LinDx):
                F, f = dx.F, dx.f
            else:
                F, f = self.linearize_dynamics(x, util.detach_maybe(u), dx, diff=False)
            if isinstance(cost, QuadCost):
                C, c = cost.C, cost.c
            else:
                C, c, _ = self.approximate_cost(x, util.detach_maybe(u), cost, diff=False)
            with torch.no_grad():
                x, u, n_qp, costs, full_du_norm, mean_alphas = self.solve_lqr_subproblem(
                    x_init, C, c, F, f, cost, dx, x, u)
            n_not_improved += 1
            assert x.ndimension() == 3 and u.ndimension() == 3
            first = best is None
            if first:
                best = dict(x=torch.empty_like(x), u=torch.empty_like(u), costs=torch.empty_like(costs),
                            full_du_norm=torch.empty_like(full_du_norm))
            any_improved, max_du = be.select_best(first, self.best_cost_eps, x.contiguous(), u.contiguous(),
                                                  costs, full_du_norm, best)
            flags = torch.stack((any_improved[0].to(max_du.dtype), max_du[0])).tolist()   # the one sync
            if self.flag_reducer is not None:
                flags = list(self.flag_reducer(flags[0] != 0, flags[1]))
            if flags[0]:
                n_not_improved = 0
            max_du_norm = flags[1]
            if self.verbose > 0:
                util.table_log("lqr", (
                    ("iter", i),
                    ("mean(cost)", best["costs"].mean().item(), "{:.4e}"),
                    ("||full_du||_max", max_du_norm, "{:.2e}"),
                    ("mean(alphas)", float(mean_alphas), "{:.2e}"),
                    ("total_qp_iters", n_qp),
                ))
            if max_du_norm < self.eps or n_not_improved > self.not_improved_lim:
                break
        return best

    def _check_converged(self, full_du_norm):
        """mpc/mpc.py:321-334: raise / warn when some problem did not reach a fixed point.  Returns
        True when the unconverged problems have to be detached."""
        if not self.detach_unconverged:
            return False
        worst = float(full_du_norm.max().item())
        if worst > self.eps:
            if self.exit_unconverged:
                raise UnconvergedError(
                    "MPC: max ||du|| = %.3e > eps = %.1e after %d LQR iterations "
                    "(exit_unconverged=True)" % (worst, self.eps, self.lqr_iter))
            if self.verbose >= 0:
                print("LQR Warning: All examples did not converge to a fixed point.")
                print("Detaching and *not* backpropping through the bad examples.")
            return True
        return False

    @staticmethod
    def _wants_graph(x_init, cost, dx):
        if not torch.is_grad_enabled():
            return False
        if x_init.requires_grad or _any_requires_grad(cost) or _any_requires_grad(dx):
            return True
        # a plain callable may close over anything: keep the reference's behaviour for those
        return not all(isinstance(z, (QuadCost, LinDx, Module)) for z in (cost, dx))

    # ------------------------------------------------------------------------------------------
    def _step_options(self):
        return StepOptions(u_lower=self.u_lower, u_upper=self.u_upper, u_zero_I=self.u_zero_I,
                           delta_u=self.delta_u, linesearch_decay=self.linesearch_decay,
                           max_linesearch_iter=self.max_linesearch_iter)

    def solve_lqr_subproblem(self, x_init, C, c, F, f, cost, dynamics, x, u, no_op_forward=False, shared_grad_kernel=False):
        """Build the LQRStep for the current nominal (x,u) and apply it (mpc/mpc.py:339-361)."""
        if self.slew_rate_penalty is not None and not isinstance(cost, Module):
            return self._solve_slew_subproblem(x_init, C, c, F, f, cost, dynamics, x, u, no_op_forward)
        step = self._lqr_step(self.n_state, cost, dynamics, x, u, no_op_forward, dict(
            c_symmetric=no_op_forward and getattr(self, "_c_symmetric", False), shared_grad_kernel=shared_grad_kernel,
            **(dict(narrow_kkt_kernel=True) if self.narrow_kkt_kernel else {}),
            **(dict(f64_grad_kernel=True) if self.f64_grad_kernel else {})))
        return step(x_init, C, c, F, f if f is not None else x_init.new_empty(0))

    def _lqr_step(self, n_state, true_cost, true_dynamics, current_x, current_u, no_op_forward, extra):
        """The LQRStep of this controller's options on `n_state` states; `extra`: the keywords only one caller passes."""
        return LQRStep(
            n_state=n_state, n_ctrl=self.n_ctrl, T=self.T, u_lower=self.u_lower, u_upper=self.u_upper, u_zero_I=self.u_zero_I,
            true_cost=true_cost, true_dynamics=true_dynamics, delta_u=self.delta_u,
            linesearch_decay=self.linesearch_decay, max_linesearch_iter=self.max_linesearch_iter,
            delta_space=True, current_x=current_x, current_u=current_u, back_eps=self.back_eps, no_op_forward=no_op_forward,
            reference_du_norm=self.reference_du_norm and not no_op_forward, **extra)

    def _solve_slew_subproblem(self, x_init, C, c, F, f, cost, dynamics, x, u, no_op_forward):
        """slew_rate_penalty: the same LQR step on the state augmented with the previous control,
        z_t = (u_{t-1}, x_t), with 0.5*gamma*|u_t - u_{t-1}|^2 added to the stage cost
        (reference mpc/mpc.py:362-445).  Pure re-packing around the kernel; autograd reaches C, c, F, f
        through the padding ops."""
        from .dynamics import CtrlPassthroughDynamics
        ns, nc = self.n_state, self.n_ctrl
        slew_C, aC, ac, aF, af = self._slew_compose(C, c, F, f)
        prev_u = self._slew_prev_u(C.size(1), dict(dtype=C.dtype, device=C.device))
        ax = torch.cat((torch.cat((prev_u, util.detach_maybe(u)[:-1])), x), 2)
        ax_init = torch.cat((prev_u[0], x_init), 1)
        a_dyn = None if isinstance(dynamics, LinDx) else CtrlPassthroughDynamics(dynamics)
        a_cost = QuadCost(aC, ac) if isinstance(cost, QuadCost) else SlewRateCost(cost, slew_C, ns, nc)
        # (`narrow_kkt_kernel` only: the promise of the plain ending, see __init__)
        extra = dict(narrow_kkt_kernel=True, c_symmetric=no_op_forward and getattr(self, "_c_symmetric", False)) if self.narrow_kkt_kernel else {}
        if self.f64_grad_kernel:
            extra["f64_grad_kernel"] = True
        step = self._lqr_step(ns + nc, a_cost, a_dyn, ax, u, no_op_forward, extra)
        out = step(ax_init, aC, ac, aF, af if af is not None else aC.new_empty(0))
        return (out[0][:, :, nc:],) + tuple(out[1:])

    def _slew_compose(self, C, c, F, f):
        """(slew_C, aC, aC's linear term ac, aF, af) of the slew-rate augmentation from [T,B,...] tensors, in torch: autograd
        reaches C, c, F, f through the padding ops.  F None (a simulator carried by the kernels): aF = af = None."""
        T, ns, nc = self.T, self.n_state, self.n_ctrl
        B = C.size(1)
        n, na = ns + nc, ns + 2 * nc
        kw = dict(dtype=C.dtype, device=C.device)
        gI = self.slew_rate_penalty * torch.eye(nc, **kw)
        slew_C = torch.zeros(T, B, na, na, **kw)
        slew_C[:, :, :nc, :nc] = gI
        slew_C[:, :, -nc:, :nc] = -gI
        slew_C[:, :, :nc, -nc:] = -gI
        slew_C[:, :, -nc:, -nc:] = gI
        aC = slew_C + torch.nn.functional.pad(C, (nc, 0, nc, 0))
        ac = torch.cat((torch.zeros(T, B, nc, **kw), c), 2)
        if F is None:
            return slew_C, aC, ac, None, None
        carry = torch.cat((torch.zeros(nc, n, **kw), torch.eye(nc, **kw)), 1)       # u_t -> next state's u_{t-1}
        aF = torch.cat((carry.expand(T - 1, B, nc, na),
                        torch.cat((torch.zeros(T - 1, B, ns, nc, **kw), F), 3)), 2)
        af = None if f is None or f.numel() == 0 else torch.cat((torch.zeros(T - 1, B, nc, **kw), f), 2)
        return slew_C, aC, ac, aF, af

    def _slew_prev_u(self, B, kw):
        """`prev_ctrl` as [1,B,n_ctrl] (every rank up to three broadcasts from the left; None = zeros)."""
        if self.prev_ctrl is not None:
            prev_u = self.prev_ctrl.detach().to(**kw)
            while prev_u.ndimension() < 3:
                prev_u = prev_u.unsqueeze(0)
        else:
            prev_u = torch.zeros(1, B, self.n_ctrl, **kw)
        return prev_u.expand(1, B, self.n_ctrl)

    # ------------------------------------------------------------------------------------------
    def approximate_cost(self, x, u, Cf, diff=True):
        """Second-order expansion of a module cost along (x,u) via autograd (mpc/mpc.py:447-487)."""
        with torch.enable_grad():
            tau = torch.cat((x, u), dim=2).detach().requires_grad_(True)
            costs, hessians, grads = [], [], []
            for t in range(self.T):
                tau_t = tau[t]
                cost = Cf(tau_t)
                grad = torch.autograd.grad(cost.sum(), tau_t, create_graph=True, retain_graph=True)[0]
                rows = [torch.autograd.grad(grad[:, j].sum(), tau_t, retain_graph=True)[0]
                        for j in range(tau.shape[2])]
                hessian = torch.stack(rows, dim=-1)
                costs.append(cost)
                grads.append(grad - util.bmv(hessian, tau_t))
                hessians.append(hessian)
            costs, grads, hessians = torch.stack(costs), torch.stack(grads), torch.stack(hessians)
            if not diff:
                return hessians.detach(), grads.detach(), costs.detach()
            return hessians, grads, costs

    def _param_grad_env(self, dynamics, x):
        """The EnvSpec of `dynamics` when its differentiable linearisation (GradMethods.AUTO_DIFF, diff=True) runs as
        _native.EnvLinearizeFn, else None (the module path through torch): a shipped simulator as it came (SimulatorDx.
        native_param_grad), `params` its only tensor that asks for a gradient, T > 1, float32 / float64, and a backend that has the
        backward (and, when it takes device tensors only, a trajectory on the device)."""
        be = _native.backend()
        fn = getattr(dynamics, "native_param_grad", None)
        if (fn is None or self.T <= 1 or not isinstance(dynamics, Module) or not hasattr(be, "env_linearize_backward")
                or x.dtype not in (torch.float32, torch.float64) or (getattr(be, "device_only", False) and not x.is_cuda)
                or not _only_params_require_grad(dynamics)):
            return None
        return fn()

    def _param_grad_net(self, dynamics, x):
        """(MlpSpec, [W_1, b_1, ...]) of `dynamics` when its differentiable linearisation (GradMethods.ANALYTIC, diff=True)
        runs as _native.MlpLinearizeFn, else None (the module path through torch): the controller was built with
        `weight_grad_kernel=True` (a float32 network) or `f64_weight_grad_kernel=True` (a float64 one), an NNDynamics the kernels
        take as it came (`native_net`: no overridden forward, no hooks, stock activations, on the device), not ELU, a network
        the weight-gradient kernel of that dtype covers (mpc_mlp_supported bit 2 / mpc_mlp_param_grad_supported_dtype), T > 1, a
        backend that has the backward of that dtype, and the `fcs` weights and biases the module's only tensors that ask for a
        gradient."""
        be = _native.backend()
        if x.dtype == torch.float64:
            # a float64 network: its own flag, its own backend method and its own query (mpc_mlp_param_grad_supported_dtype)
            on, method = self.f64_weight_grad_kernel, "mlp_linearize_backward64"
        else:
            on, method = self.weight_grad_kernel and x.dtype == torch.float32, "mlp_linearize_backward"
        if (not on or self.T <= 1 or not isinstance(dynamics, Module) or not hasattr(dynamics, "native_net") or not hasattr(dynamics, "fcs")
                or not hasattr(be, method)):
            return None
        net = dynamics.native_net(x)
        if net is None or net.activation == "elu" or net.ctrl_carry:
            return None
        if not (net.param_grad_supported(torch.float64) if x.dtype == torch.float64 else net.param_grad_supported()):
            return None
        params = [t for layer in dynamics.fcs for t in (layer.weight, layer.bias)]
        if len(params) != 2 * len(net.weights) or any(a is not b for a, b in zip(params[0::2], net.weights)) \
                or any(a is not b for a, b in zip(params[1::2], net.biases)):
            return None
        if any(not any(t is p for p in params) for t in _grad_tensors(dynamics)):
            return None
        return net, params

    def linearize_dynamics(self, x, u, dynamics, diff):
        """F_t = [df/dx | df/du], f_t = f(x_t,u_t) - F_t [x_t;u_t] along the trajectory
        (mpc/mpc.py:490-601).  ANALYTIC uses the module's grad_input over all (T-1)*B points at
        once; AUTO_DIFF batches the reference's (T-1)*n_state backward passes into n_state."""
        T, ns, nc = self.T, self.n_state, self.n_ctrl
        B = x.shape[1]
        if self.grad_method == GradMethods.ANALYTIC:
            net = dynamics.native_net(x) if (not diff and hasattr(dynamics, "native_net") and T > 1) else None
            if net is not None and net.activation != "elu":
                # NNDynamics: forward, grad_input and the affine term in one kernel, no [N, hidden, n] intermediates
                # (elu has no grad_input in the reference, mpc/dynamics.py:113-114: left to the module to refuse)
                Fl, fl = _native.backend().mlp_linearize(net, x[:-1].reshape(-1, ns), u[:-1].reshape(-1, nc))
                return Fl.view(T - 1, B, ns, ns + nc), fl.view(T - 1, B, ns)
            routed = self._param_grad_net(dynamics, x) if diff else None
            if routed is not None:
                # a trainable NNDynamics: the linearisation kernel forward, its weight-gradient kernel backward (x, u constants
                # as below) -- not the module over all points with [N, hidden, n] intermediates and an autograd pass through them
                with torch.enable_grad():
                    Fl, fl = _native.MlpLinearizeFn.apply(routed[0], x[:-1].reshape(-1, ns).detach(), u[:-1].reshape(-1, nc).detach(),
                                                          *routed[1])
                return Fl.view(T - 1, B, ns, ns + nc), fl.view(T - 1, B, ns)
            # fresh leaves, as the reference (mpc/mpc.py:495-497): with diff=True the graph reaches the
            # dynamics' parameters (through new_x, R, S), not the trajectory itself.
            _x = x[:-1].reshape(-1, ns).detach().requires_grad_(True)
            _u = u[:-1].reshape(-1, nc).detach().requires_grad_(True)
            new_x = dynamics(_x, _u)
            if not diff:
                new_x, _x, _u = new_x.detach(), _x.detach(), _u.detach()
            R, S = dynamics.grad_input(_x, _u)
            f = (new_x - util.bmv(R, _x) - util.bmv(S, _u)).view(T - 1, B, ns)
            F = torch.cat((R.reshape(T - 1, B, ns, ns), S.reshape(T - 1, B, ns, nc)), 3)
            return F, f
        if self.grad_method == GradMethods.AUTO_DIFF:
            env = self._param_grad_env(dynamics, x) if diff else None
            if env is not None:
                # a shipped simulator whose parameters are being learned: closed-form kernel forward, its parameter
                # gradient kernel backward (x, u constants as below) -- not n_state double-backward passes through torch
                with torch.enable_grad():
                    Fl, fl = _native.EnvLinearizeFn.apply(dynamics.params, env, x[:-1].reshape(-1, ns).detach(),
                                                          u[:-1].reshape(-1, nc).detach())
                return Fl.view(T - 1, B, ns, ns + nc), fl.view(T - 1, B, ns)
            with torch.enable_grad():
                xt = x[:-1].reshape(-1, ns).detach().requires_grad_(True)
                ut = u[:-1].reshape(-1, nc).detach().requires_grad_(True)
                new_x = dynamics(xt, ut)
                Rs, Ss = [], []
                for j in range(ns):      # n_state backward passes over ALL (T-1)*B points at once
                    Rj, Sj = torch.autograd.grad(new_x[:, j].sum(), [xt, ut], retain_graph=True,
                                                 create_graph=diff)
                    Rs.append(Rj)
                    Ss.append(Sj)
                R, S = torch.stack(Rs, 1), torch.stack(Ss, 1)
                if not diff:
                    new_x, xt, ut, R, S = (z.detach() for z in (new_x, xt, ut, R, S))
                f = (new_x - util.bmv(R, xt) - util.bmv(S, ut)).view(T - 1, B, ns)
                F = torch.cat((R, S), 2).view(T - 1, B, ns, ns + nc)
            return F, f
        if self.grad_method == GradMethods.FINITE_DIFF:
            eps = 1e-4
            xt = x[:-1].reshape(-1, ns).detach()
            ut = u[:-1].reshape(-1, nc).detach()
            with torch.no_grad():
                new_x = dynamics(xt, ut)
                cols = []
                for j in range(ns + nc):
                    e = torch.zeros(ns + nc, dtype=xt.dtype, device=xt.device)
                    e[j] = eps
                    hi = dynamics(xt + e[:ns], ut + e[ns:])
                    lo = dynamics(xt - e[:ns], ut - e[ns:])
                    cols.append((hi - lo) / (2. * eps))
                Fm = torch.stack(cols, 2)
                f = (new_x - util.bmv(Fm, torch.cat((xt, ut), 1))).view(T - 1, B, ns)
            return Fm.view(T - 1, B, ns, ns + nc), f
        assert False
