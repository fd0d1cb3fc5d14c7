"""GPU tests (-m gpu) of mpc_lqr_kkt_grads_shared (csrc/kkt_shared.hip) and of `shared_grad_kernel=` on the device.

1. The entry against the existing one on the same inputs.  Reference: mpc_lqr_kkt_grads' per-problem dC, dc, dF, df, added over
   the batch in float64 on the host.  Bound per entry: |got - ref| <= (B + 2) 2^-24 S, with S the float64 sum over the batch of
   the absolute values of the products that make up the entry -- the a-priori bound for any order of B float32 additions of
   fma-rounded terms (3e-7 S at B = 3, which a reduced-precision MFMA would miss by orders of magnitude; 6e-5 S at B = 1030).
   Each case prints its largest ratio err / bound and, next to it, the same ratio of the parent's float32 `.sum(1)`.
   dx_init is bitwise the existing entry's, two runs are bitwise equal, NULL outputs are honoured.

   n_state = 12, n_ctrl = 4: on 16-byte aligned buffers mpc_lqr_kkt_grads runs that shape on the 4-problems-per-wave kernel,
   whose costate recursion sums on two interleaved chains -- other roundings than kkt_costate_kernel's single chain, which
   the batch-summed route is built on (and which a sum-order bound does not cover: the two differ in lambda itself).  The
   reference of that shape therefore runs the existing entry on the wavefront-per-problem kernels, which it takes by itself
   for a dC that is not 16-byte aligned; test_the_12_4_kernel_of_the_existing_entry holds the two recursions together on
   aligned buffers.
2. The costate kernel's parking stride: lambda, dlambda in the compact area are bitwise what the existing route parks in the
   dF blocks, read through df = -dlambda and a column of dF that is -lambda exactly (u* = 0 and du = 1 in the last control).
3. Whole solves through mpc.MPC, float32 against the float64 solve with the flag off.
"""
import ctypes

import pytest
import torch

from mpc import _native, mpc
from mpc.mpc import LinDx, QuadCost

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load()
    return _native.HipBackend()


def make_inputs(ns, nc, B, T, share, with_f, bounds, seed):
    """C, c, F, f as [T,B,...] views (share: "BT" = stride 0 over batch and time, "B" = over the batch, "none" = per problem),
    a trajectory (x*, u*) with about a third of the controls on a bound when `bounds`, and cotangents dl_dx, dl_du."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    n = ns + nc
    lead = {"BT": ((), ()), "B": ((T,), (T - 1,)), "none": ((T, B), (T - 1, B))}[share]
    L = r(*lead[0], n, n) / n ** 0.5
    C = L.transpose(-1, -2) @ L + torch.eye(n)
    C = 0.5 * (C + C.transpose(-1, -2))
    c = r(*lead[0], n)
    F = torch.cat((0.9 * torch.eye(ns).expand(*lead[1], ns, ns) + 0.3 * r(*lead[1], ns, ns) / ns ** 0.5, 0.5 * r(*lead[1], ns, nc)), -1)
    f = 0.2 * r(*lead[1], ns) if with_f else None

    def view(t, steps, inner):
        if t is None:
            return None
        t = t.to(DEV)
        if share == "BT":
            return t.expand(steps, B, *inner)
        if share == "B":
            return t.unsqueeze(1).expand(steps, B, *inner)
        return t
    xs, us = r(T, B, ns), r(T, B, nc).clamp(-1.0, 1.0)
    opts = _native.StepOptions()
    if bounds:
        pick = torch.rand(T, B, nc, generator=g)
        us = torch.where(pick < 1 / 6, torch.full_like(us, -0.7), torch.where(pick > 5 / 6, torch.full_like(us, 0.7), us.clamp(-0.69, 0.69)))
        opts = _native.StepOptions(u_lower=-0.7, u_upper=0.7)
    return dict(C=view(C, T, (n, n)), c=view(c, T, (n,)), F=view(F, T - 1, (ns, n)), f=view(f, T - 1, (ns,)), xs=xs.to(DEV), us=us.to(DEV),
                dl_dx=r(T, B, ns).to(DEV), dl_du=r(T, B, nc).to(DEV), opts=opts, ns=ns, nc=nc, B=B, T=T)


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def call_existing(be, z, dx, du, off_grid=False):
    """mpc_lqr_kkt_grads itself, every output pre-filled with NaN.  off_grid: dC starts 4 bytes off the 16-byte grid."""
    L = _native.load()
    T, B, ns, nc = z["T"], z["B"], z["ns"], z["nc"]
    n = ns + nc
    p, keep = be._problem(z["xs"][0], z["C"], z["c"], z["F"], z["f"], z["xs"], z["us"])
    dC = nan(T * B * n * n + 4)[1 if off_grid else 0:][:T * B * n * n].view(T, B, n, n)
    dc, dF, dx_init = nan(T, B, n), nan(max(T - 1, 0), B, ns, n), nan(B, ns)
    df = nan(T - 1, B, ns) if (z["f"] is not None and T > 1) else None
    rc = L.mpc_lqr_kkt_grads(ctypes.byref(p), dx.data_ptr(), du.data_ptr(), z["dl_dx"].data_ptr(), z["dl_du"].data_ptr(), dC.data_ptr(),
                             dc.data_ptr(), dF.data_ptr() if T > 1 else None, _native._ptr(df), dx_init.data_ptr(), _native._stream(dx.device))
    assert rc == 0, L.mpc_lqr_last_error()
    torch.cuda.synchronize()
    return dict(dC=dC, dc=dc, dF=dF, df=df, dx_init=dx_init)


def call_shared(be, z, dx, du, want=(True, True, True, True)):
    """mpc_lqr_kkt_grads_shared itself, outputs and workspace pre-filled with NaN."""
    L = _native.load()
    T, B, ns, nc = z["T"], z["B"], z["ns"], z["nc"]
    n = ns + nc
    p, keep = be._problem(z["xs"][0], z["C"], z["c"], z["F"], z["f"], z["xs"], z["us"])
    assert L.mpc_lqr_kkt_shared_supported(ctypes.byref(p)) == 1
    nbytes = int(L.mpc_lqr_kkt_shared_workspace_bytes(ctypes.byref(p)))
    ws = nan(nbytes // 4)
    want = (want[0], want[1], want[2] and T > 1, want[3] and T > 1 and z["f"] is not None)
    shapes = ((T, n, n), (T, n), (T - 1, ns, n), (T - 1, ns))
    sums = [nan(*s) if w else None for s, w in zip(shapes, want)]
    dx_init = nan(B, ns)
    rc = L.mpc_lqr_kkt_grads_shared(ctypes.byref(p), dx.data_ptr(), du.data_ptr(), z["dl_dx"].data_ptr(), z["dl_du"].data_ptr(),
                                    *[_native._ptr(s) for s in sums], dx_init.data_ptr(), ws.data_ptr(), nbytes, _native._stream(dx.device))
    assert rc == 0, L.mpc_lqr_last_error()
    torch.cuda.synchronize()
    return dict(sum_dC=sums[0], sum_dc=sums[1], sum_dF=sums[2], sum_df=sums[3], dx_init=dx_init, ws=ws)


def costates64(z, dx, du):
    """lambda_{t+1}, dlambda_{t+1} [T-1,B,ns] by the recursion of mpc/lqr_step.py:355-385 in float64 (for the bound's S only)."""
    T, ns = z["T"], z["ns"]
    C, c, F = z["C"].double(), z["c"].double(), (z["F"].double() if T > 1 else None)
    tau, d = torch.cat((z["xs"], z["us"]), 2).double(), torch.cat((dx, du), 2).double()
    lam, dlam, out_l, out_d = None, None, [], []
    for t in range(T - 1, -1, -1):
        l = torch.einsum("bij,bj->bi", C[t][:, :ns], tau[t]) + c[t][:, :ns]
        dl = torch.einsum("bij,bj->bi", C[t][:, :ns], d[t]) - z["dl_dx"][t].double()
        if t < T - 1:
            l = l + torch.einsum("bmi,bm->bi", F[t][:, :, :ns], lam)
            dl = dl + torch.einsum("bmi,bm->bi", F[t][:, :, :ns], dlam)
            out_l.append(lam); out_d.append(dlam)
        lam, dlam = l, dl
    if T == 1:
        return None, None
    return torch.stack(out_l[::-1]), torch.stack(out_d[::-1])


def scales(z, dx, du):
    """S of every entry of the four sums: the float64 sum over the batch of the absolute products behind it."""
    X, D = torch.cat((z["xs"], z["us"]), 2).double().abs(), torch.cat((dx, du), 2).double().abs()
    S = dict(sum_dC=0.5 * (torch.einsum("tbi,tbj->tij", D, X) + torch.einsum("tbi,tbj->tij", X, D)), sum_dc=D.sum(1))
    lam, dlam = costates64(z, dx, du)
    if lam is not None:
        S["sum_dF"] = torch.einsum("tbi,tbj->tij", dlam.abs(), X[:-1]) + torch.einsum("tbi,tbj->tij", lam.abs(), D[:-1])
        S["sum_df"] = dlam.abs().sum(1)
    return S


NAMES = (("sum_dC", "dC"), ("sum_dc", "dc"), ("sum_dF", "dF"), ("sum_df", "df"))


def ratios(z, got, old, S):
    """max over the entries of |sum - ref| / ((B + 2) 2^-24 S) for the entry's sums and for the parent's float32 .sum(1)"""
    out = {}
    for new, src in NAMES:
        if got[new] is None:
            continue
        ref = old[src].double().sum(1)
        bound = (z["B"] + 2) * U * S[new]
        assert torch.isfinite(got[new]).all(), new
        bound = bound.clamp_min(1e-300)          # (an entry without terms: both sides are exact zeros)
        out[new] = (float(((got[new].double() - ref).abs() / bound).max()), float(((old[src].sum(1).double() - ref).abs() / bound).max()))
    return out


#         ns  nc     B  T share  f      bounds
CASES = ((3, 1, 3, 9, "BT", True, False),
         (3, 1, 1030, 2, "B", False, True),
         (12, 4, 67, 9, "B", True, True),              # one tile exactly
         (12, 4, 1030, 2, "BT", False, False),
         (13, 4, 67, 9, "none", True, False),          # n = 17: a ragged second tile
         (13, 4, 1, 1, "B", False, False),
         (10, 3, 1030, 9, "B", True, True),            # off the 16-byte grid; 33 chunks on 32 partials: block 0 takes two
         (10, 3, 2100, 2, "BT", True, False),          # 66 chunks on 32 partials: two or three chunks a block
         (32, 8, 67, 9, "BT", True, True),
         (32, 8, 3, 2, "none", True, False),
         (45, 19, 3, 2, "none", True, False),          # n = 64
         (45, 19, 67, 9, "B", False, True),
         (63, 1, 67, 2, "BT", True, True),
         (63, 1, 1, 9, "B", True, False))


@pytest.mark.parametrize("ns,nc,B,T,share,with_f,bounds", CASES)
def test_entry_against_the_existing_one(be, ns, nc, B, T, share, with_f, bounds):
    z = make_inputs(ns, nc, B, T, share, with_f, bounds, seed=1000 * ns + B + T)
    # (dx, du) of the KKT solve: mpc_lqr_kkt_prepare and the nested step, as every caller of either entry has them
    Fz = z["F"] if T > 1 else torch.empty(0, B, ns, ns + nc, device=DEV)
    first = be.kkt_backward_shared(z["C"], z["c"], Fz, z["f"], z["xs"], z["us"], z["dl_dx"], z["dl_du"], z["opts"])
    dx, du = first["dx"], first["du"]
    if bounds:
        pinned = (z["us"].abs() == 0.7)
        assert 0.25 < float(pinned.float().mean()) < 0.42 and bool((du[pinned] == 0).all())
    old = call_existing(be, z, dx, du, off_grid=(ns, nc) == (12, 4))
    got = call_shared(be, z, dx, du)
    assert got["sum_dF"] is None or T > 1
    assert (got["sum_df"] is None) == (not with_f or T == 1)
    for k, v in ratios(z, got, old, scales(z, dx, du)).items():
        print("%d/%d B=%d T=%d %s %s: err / bound  new %.2e  float32 .sum(1) %.2e" % (ns, nc, B, T, share, k, v[0], v[1]))
        assert v[0] <= 1.0, (k, v)
    assert torch.equal(got["dx_init"], old["dx_init"])
    assert torch.equal(got["sum_dC"], got["sum_dC"].transpose(1, 2))
    # the Python front hands out the same numbers
    for k in ("sum_dC", "sum_dc", "sum_dF", "sum_df", "dx_init"):
        assert (first[k] is None and got[k] is None) or torch.equal(first[k], got[k]), k
    # twice the same bits, whatever the outputs and the workspace held before
    again = call_shared(be, z, dx, du)
    for k in ("sum_dC", "sum_dc", "sum_dF", "sum_df", "dx_init"):
        assert (again[k] is None and got[k] is None) or torch.equal(again[k], got[k]), k
    # NULL outputs are honoured
    if T > 1:
        only = call_shared(be, z, dx, du, want=(False, False, True, False))
        assert torch.equal(only["sum_dF"], got["sum_dF"]) and torch.equal(only["dx_init"], got["dx_init"])
    only = call_shared(be, z, dx, du, want=(False, True, False, False))
    assert torch.equal(only["sum_dc"], got["sum_dc"])


def test_the_12_4_kernel_of_the_existing_entry(be):
    """On aligned buffers mpc_lqr_kkt_grads takes n_state = 12, n_ctrl = 4 to the 4-problems-per-wave kernel.  Its costates
    and kkt_costate_kernel's are the same recursion in another order of additions, so dx_init agrees to rounding, not
    bitwise: each costate is a sum of n + n_state = 28 products on top of the next one, T of them deep, so either order is
    within T (n + n_state) 2^-24 of the recursion's sum of absolute terms (propagated through |F_x|), the two within twice that."""
    z = make_inputs(12, 4, 67, 9, "B", True, True, seed=12067)
    first = be.kkt_backward_shared(z["C"], z["c"], z["F"], z["f"], z["xs"], z["us"], z["dl_dx"], z["dl_du"], z["opts"])
    dx, du = first["dx"], first["du"]
    old = call_existing(be, z, dx, du)
    wave = call_existing(be, z, dx, du, off_grid=True)
    got = call_shared(be, z, dx, du)
    assert torch.equal(got["dx_init"], wave["dx_init"])
    diff, scale = float((old["dx_init"] - wave["dx_init"]).abs().max()), float(costate_scale(z, dx, du))
    print("12/4 dx_init: the two recursions differ by %.3g x 2^-24 x scale" % (diff / (U * scale)))
    assert diff <= 2 * z["T"] * 28 * U * scale


def costate_scale(z, dx, du):
    """max over problems and states of the sum of |terms| of dlambda_0's recursion, float64"""
    T, ns = z["T"], z["ns"]
    C, F = z["C"].double().abs(), z["F"].double().abs()
    d = torch.cat((dx, du), 2).double().abs()
    acc = None
    for t in range(T - 1, -1, -1):
        a = torch.einsum("bij,bj->bi", C[t][:, :ns], d[t]) + z["dl_dx"][t].double().abs()
        if acc is not None:
            a = a + torch.einsum("bmi,bm->bi", F[t][:, :, :ns], acc)
        acc = a
    return acc.max()


@pytest.mark.parametrize("ns,nc", ((12, 4), (13, 4)))
def test_costates_in_the_compact_area_are_the_parked_ones(be, ns, nc):
    """kkt_costate_kernel with the parking stride 2 n_state (the workspace's [T-1,B,2 n_state] area) against the stride
    n_state n of the existing route (the dF blocks, which the outer-product kernel then overwrites): dlambda through
    df = -dlambda, lambda through the last column of dF, which is -(dlambda u* + lambda du) = -lambda exactly where the last
    control has u* = 0 and du = 1."""
    T, B = 9, 67
    z = make_inputs(ns, nc, B, T, "B", True, False, seed=77 + ns)
    g = torch.Generator().manual_seed(5)
    dx, du = torch.randn(T, B, ns, generator=g).to(DEV), torch.randn(T, B, nc, generator=g).to(DEV)
    z["us"][:, :, -1] = 0.0
    du[:, :, -1] = 1.0
    old = call_existing(be, z, dx, du, off_grid=(ns, nc) == (12, 4))        # (12/4: the wavefront-per-problem kernels, see above)
    got = call_shared(be, z, dx, du)
    parked = got["ws"][:(T - 1) * B * 2 * ns].view(T - 1, B, 2, ns)
    assert torch.isfinite(parked).all()
    assert torch.equal(parked[:, :, 1], -old["df"])
    assert torch.equal(parked[:, :, 0], -old["dF"][:, :, :, -1])
    assert torch.equal(got["dx_init"], old["dx_init"])


# ---------------------------------------------------------------------------------------------
# 3. whole solves
# ---------------------------------------------------------------------------------------------
def shared_problem(ns, nc, T, B, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    n = ns + nc
    L = r(T, n, n) / n ** 0.5
    C = L.transpose(1, 2) @ L + torch.eye(n, dtype=torch.float64)
    F = torch.cat((0.9 * torch.eye(ns, dtype=torch.float64).expand(T - 1, ns, ns) + 0.3 * r(T - 1, ns, ns) / ns ** 0.5, 0.5 * r(T - 1, ns, nc)), 2)
    return dict(C=0.5 * (C + C.transpose(1, 2)), c=r(T, n), F=F, f=0.2 * r(T - 1, ns), x_init=r(B, ns), wx=r(T, B, ns), wu=r(T, B, nc))


def solve_and_grads(p, ns, nc, T, B, dtype, flag, bounded):
    leaves = [p[k].to(device=DEV, dtype=dtype).requires_grad_(True) for k in ("C", "c", "F", "f")]
    kw = dict(u_lower=-0.5, u_upper=0.5) if bounded else {}
    ctrl = mpc.MPC(ns, nc, T, lqr_iter=3, verbose=-1, exit_unconverged=False, detach_unconverged=False, n_batch=B,
                   shared_grad_kernel=flag, **kw)
    x, u, costs = ctrl(p["x_init"].to(device=DEV, dtype=dtype), QuadCost(leaves[0], leaves[1]), LinDx(leaves[2], leaves[3]))
    loss = (x * p["wx"].to(device=DEV, dtype=dtype)).sum() + (u * p["wu"].to(device=DEV, dtype=dtype)).sum()
    grads = torch.autograd.grad(loss, leaves)
    assert all(g.shape == l.shape for g, l in zip(grads, leaves))
    return [g.double() for g in grads], x.detach(), u.detach(), costs.detach()


@pytest.mark.parametrize("bounded", (True, False))
@pytest.mark.parametrize("ns,nc,T,B", ((12, 4, 10, 67), (20, 5, 8, 33)))
def test_whole_solves_with_a_shared_learnable_cost_and_model(be, monkeypatch, ns, nc, T, B, bounded):
    """err = max-norm error of a gradient relative to its max-norm, against the float64 solve with the flag off: the two
    float32 routes differ only in the order of a sum and share the float32 KKT solve that dominates both errors, so
    err_new <= 4 err_old + 1e-6."""
    calls = []
    for name in ("kkt_backward", "kkt_backward_shared"):
        orig = getattr(_native.HipBackend, name)
        monkeypatch.setattr(_native.HipBackend, name, (lambda o, nm: lambda self, *a, **k: (calls.append(nm), o(self, *a, **k))[1])(orig, name))
    p = shared_problem(ns, nc, T, B, seed=ns + B)
    ref, x64, u64, _ = solve_and_grads(p, ns, nc, T, B, torch.float64, False, bounded)
    assert calls == ["kkt_backward"]
    del calls[:]
    new, xn, un, cn = solve_and_grads(p, ns, nc, T, B, torch.float32, True, bounded)
    assert calls == ["kkt_backward_shared"]
    old, xo, uo, co = solve_and_grads(p, ns, nc, T, B, torch.float32, False, bounded)
    assert torch.equal(xn, xo) and torch.equal(un, uo) and torch.equal(cn, co)          # the iterations are untouched
    for k, gn, go, gr in zip("CcFf", new, old, ref):
        err_new, err_old = float((gn - gr).abs().max() / gr.abs().max()), float((go - gr).abs().max() / gr.abs().max())
        print("%d/%d T=%d B=%d %s d%s: err_new %.3e err_old %.3e" % (ns, nc, T, B, "box" if bounded else "free", k, err_new, err_old))
        assert err_new <= 4 * err_old + 1e-6, (k, err_new, err_old)
    # float64 with the flag on: kkt_backward_shared's own fallback (kkt_backward, then the sum over the batch)
    del calls[:]
    on64, x64n, u64n, _ = solve_and_grads(p, ns, nc, T, B, torch.float64, True, bounded)
    assert calls == ["kkt_backward_shared", "kkt_backward"]
    assert torch.equal(x64n, x64) and torch.equal(u64n, u64)
    for gn, gr in zip(on64, ref):
        assert float((gn - gr).abs().max()) <= 1e-9 * max(1.0, float(gr.abs().max()))
