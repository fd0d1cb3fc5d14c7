"""GPU (-m gpu): the launch shapes the host-side plan of the NNDynamics kernels chooses (csrc/nn_dynamics.hip: nn_plan --
wavefronts per workgroup nw, grid, dynamic LDS, weights staged or read from global memory), at the group counts where
the plan changes: 1024 / 2048 / 4096 groups of sixteen problems, one group short of them, ragged tails.

Two kinds of assertion on every large call:

  1. bitwise -- a wavefront's arithmetic for its sixteen problems does not depend on nw or the grid, so the rows of the
     first three groups, of a middle group and of the last (ragged) group equal, bit for bit, the same rows computed by a
     small call (nw = 1) on that slice alone;
  2. every row against the float64 oracle (oracle/env_oracle.py), with the tolerances
     tests/test_gpu_nn.py::test_network_rollout_and_linearisation_at_full_batches uses for the same quantities.

The plan's arithmetic for the two (12, 4) networks, from the formulas of nn_plan (wp = widths rounded up to 16):
  [16, 100, 100, 12]: packed 112*20+112 + 112*116+112 + 16*116+16 = 17,328 floats = 69,312 bytes <= 96 KiB: staged; the
      Jacobian's wave area 16*20 + 2*16*116 + 2*7*256 = 7,616 floats = 30,464 bytes; at >= 4096 groups nw = 8 -> 2
      (69,312 + 2*30,464 = 130,240 bytes of dynamic LDS, past 64 KiB; nw = 4 would need 191,168 > 160 KiB)
  [16, 256, 100, 12]: packed 256*20+256 + 112*260+112 + 16*116+16 = 36,480 floats = 145,920 bytes > 96 KiB: read from global
      memory; wave area 16*20 + 2*16*260 + 2*16*256 = 16,832 floats = 67,328 bytes; nw = 8 -> 2 (134,656 bytes)

A relu network's Jacobian jumps where a hidden unit's pre-activation changes sign.  A row where the float64 pre-activation
of some unit is within the float32 forward error bound of zero (gamma_n = (n + 2) 2^-23 times the sum of absolute terms,
propagated through the layers) has two legitimate Jacobians; such rows are named from the oracle alone, must be rare
(< 1 %: the worst-case bound names a few in a thousand), and are left out of the F / f comparison with the oracle -- the bitwise comparison covers every row it touches."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from test_gpu_fullsize import host
from test_gpu_nn import f32, random_net, spec_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from mpc import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()            # fail loudly if the extension is missing
    return _native.HipBackend()


def slices(N):
    """The first three groups, a middle group, the last (ragged) group."""
    groups = (N + 15) // 16
    return [(0, 48), (16 * (groups // 2), 16 * (groups // 2) + 16), (16 * (groups - 1), N)]


def oracle_linearize(net, x, u, chunk=1024):
    """E.linearize on every row; in chunks (its [N, hidden, n] intermediates) and on threads (numpy releases the GIL)."""
    from oracle import env_oracle as E
    from oracle import lqr_oracle as O
    with ThreadPoolExecutor(max(1, min(16, O.max_threads()))) as ex:
        parts = list(ex.map(lambda a: E.linearize(E.MLP, x[a:a + chunk], u[a:a + chunk], net), range(0, len(x), chunk)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def relu_kink_rows(net, x, u):
    """Rows at which float32 cannot tell the sign of some hidden pre-activation (see the module docstring)."""
    z = np.concatenate((x, u), 1).astype(np.float64)
    err, bad = np.zeros_like(z), np.zeros(len(z), dtype=bool)
    for W, b in zip(net.Ws[:-1], net.bs[:-1]):
        pre = z @ W.T + b
        err = err @ np.abs(W).T + (W.shape[1] + 2) * 2.0 ** -23 * (np.abs(z) @ np.abs(W).T + np.abs(b))
        bad |= (np.abs(pre) <= err).any(1)
        z = np.maximum(pre, 0.0)
    return bad


LINEARIZE = [(5, 1, [64, 48], "relu", N) for N in (16 * 1023 + 7, 16 * 1024, 16 * 2048 + 1, 16 * 4096 + 5)] + [
    (20, 3, [40], "sigmoid", 16 * 1024),             # two state tiles
    (12, 4, [100, 100], "sigmoid", 16 * 4096 + 5),    # weights staged, nw 8 -> 2, more than 64 KiB of dynamic LDS
    (12, 4, [256, 100], "sigmoid", 16 * 4096 + 5),    # weights from global memory, nw 8 -> 2
]


@pytest.mark.parametrize("ns,nc,hidden,act,N", LINEARIZE)
def test_linearisation_does_not_depend_on_the_launch_shape(be, ns, nc, hidden, act, N):
    net = random_net(ns, nc, hidden, act, True, seed=ns * 100 + nc, scale=0.8)
    sp = spec_of(net)
    rng = np.random.RandomState(N % 1000 + ns)
    x, u = rng.randn(N, ns).astype(np.float32), (0.5 * rng.randn(N, nc)).astype(np.float32)
    xd, ud = f32(x), f32(u)
    F, f = be.mlp_linearize(sp, xd, ud)
    for a, b in slices(N):
        Fs, fs = be.mlp_linearize(sp, xd[a:b].contiguous(), ud[a:b].contiguous())
        assert torch.equal(F[a:b], Fs) and torch.equal(f[a:b], fs), (a, b)
    Fo, fo = oracle_linearize(net, x, u)
    keep = ~relu_kink_rows(net, x, u) if act == "relu" else np.ones(N, dtype=bool)
    print("rows left out at a relu kink: %d of %d" % (N - keep.sum(), N))
    assert N - keep.sum() < 1e-2 * N
    scale = 1.0 + np.abs(x).max()
    np.testing.assert_allclose(host(F)[keep], Fo[keep], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(host(f)[keep], fo[keep], rtol=1e-3, atol=1e-4 * scale)


def test_carry_linearisation_does_not_depend_on_the_launch_shape(be):
    """mlp_linearize_carry at 1024 groups (nw = 2): the same kernels writing the slew-rate augmentation's layout; every row
    against the oracle through that layout, aF = [[0 0 I], [0 F]], af = [0; f]."""
    ns, nc, N = 5, 1, 16 * 1024
    net = random_net(ns, nc, [64, 48], "sigmoid", True, seed=501, scale=0.8)
    sp = spec_of(net)
    rng = np.random.RandomState(3)
    z, u = rng.randn(N, nc + ns).astype(np.float32), (0.5 * rng.randn(N, nc)).astype(np.float32)
    zd, ud = f32(z), f32(u)
    aF, af = be.mlp_linearize_carry(sp, zd, ud)
    for a, b in slices(N):
        Fs, fs = be.mlp_linearize_carry(sp, zd[a:b].contiguous(), ud[a:b].contiguous())
        assert torch.equal(aF[a:b], Fs) and torch.equal(af[a:b], fs), (a, b)
    Fo, fo = oracle_linearize(net, z[:, nc:], u)
    want_F, want_f = np.zeros((N, ns + nc, ns + 2 * nc)), np.zeros((N, ns + nc))
    want_F[:, :nc, ns + nc:] = np.eye(nc)
    want_F[:, nc:, nc:] = Fo
    want_f[:, nc:] = fo
    scale = 1.0 + np.abs(z).max()
    np.testing.assert_allclose(host(aF), want_F, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(host(af), want_f, rtol=1e-3, atol=1e-4 * scale)


ROLLOUT = [(5, 1, [64, 48], 16 * 1024), (5, 1, [64, 48], 16 * 2048 + 3), (20, 3, [40], 16 * 1024)]


@pytest.mark.parametrize("ns,nc,hidden,B", ROLLOUT)
def test_rollouts_do_not_depend_on_the_launch_shape(be, ns, nc, hidden, B):
    """mlp_traj_cost with a cost (every row against E.traj / E.quad_cost) and, for the one-tile network, the line-searched
    mlp_rollout around it with small random gains and scalar bounds: the general rollout kernel at nw = 2 and nw = 4.
    The linear cost term is kept small against the positive definite one so that a relative tolerance on the cost means
    something on every one of the rows."""
    from mpc._native import StepOptions
    from oracle import env_oracle as E
    T, n, bound = 3, ns + nc, 0.5
    net = random_net(ns, nc, hidden, "sigmoid", True, seed=ns * 100 + nc, scale=0.8)
    sp = spec_of(net)
    rng = np.random.RandomState(B % 1000 + ns)
    x0 = rng.randn(B, ns).astype(np.float32)
    u0 = np.clip(0.3 * rng.randn(T, B, nc), -bound, bound).astype(np.float32)
    A = rng.randn(T, B, n, n)
    C = (np.einsum("tbki,tbkj->tbij", A, A) + 0.1 * np.eye(n)).astype(np.float32)
    c = (0.1 * rng.randn(T, B, n)).astype(np.float32)
    x0d, u0d, Cd, cd = f32(x0), f32(u0), f32(C), f32(c)
    xk, ck = be.mlp_traj_cost(x0d, u0d, sp, C=Cd, c=cd)
    cut = lambda t, a, b: t[:, a:b].contiguous()
    for a, b in slices(B):
        xs_, cs_ = be.mlp_traj_cost(x0d[a:b].contiguous(), cut(u0d, a, b), sp, C=cut(Cd, a, b), c=cut(cd, a, b))
        assert torch.equal(xk[:, a:b], xs_) and torch.equal(ck[a:b], cs_), (a, b)
    xs = E.traj(E.MLP, x0.astype(np.float64), u0.astype(np.float64), net)
    scale = 1.0 + np.abs(xs).max()
    assert np.abs(host(xk) - xs).max() < 2e-4 * scale
    np.testing.assert_allclose(host(ck), E.quad_cost(C.astype(np.float64), c.astype(np.float64), xs, u0.astype(np.float64)), rtol=1e-3)
    if ns > 16:
        return
    K, k = f32(0.05 * rng.randn(T, B, nc, ns)), f32(0.1 * rng.randn(T, B, nc))
    opts = StepOptions(u_lower=-bound, u_upper=bound, linesearch_decay=0.2, max_linesearch_iter=4)
    r = be.mlp_rollout(x0d, Cd, cd, K, k, xk, u0d, ck, opts, sp)
    for a, b in slices(B):
        s = be.mlp_rollout(x0d[a:b].contiguous(), cut(Cd, a, b), cut(cd, a, b), cut(K, a, b), cut(k, a, b), cut(xk, a, b),
                           cut(u0d, a, b), ck[a:b].contiguous(), opts, sp)
        for key in ("new_x", "new_u"):
            assert torch.equal(r[key][:, a:b], s[key]), (key, a, b)
        for key in ("costs", "alphas", "full_du_norm", "alpha_du_norm", "status"):
            assert torch.equal(r[key][a:b], s[key]), (key, a, b)
    assert (host(r["new_u"]) >= -bound - 1e-6).all() and (host(r["new_u"]) <= bound + 1e-6).all()
