"""Shared by tests/test_nn_weight_grad.py and tests/test_gpu_nn_weight_grad.py: the float64 yardstick of the NNDynamics
linearisation's weight gradient -- the recursion of include/mpc_lqr.h (mpc_mlp_param_grad) written out in torch, point by
point, so that next to every sum g_k it can hand back scale_k = sum over the points of |that point's contribution| --
and the networks and random points the kernel is run on.  tests/test_nn_weight_grad.py holds it to the reference-made
fixture and to float64 autograd of the package's own module at 1e-9 of scale."""
import math

import torch

F64 = torch.float64
REL_H = 1e-3          # relu: a kept point has |h| >= REL_H at every hidden unit (a slope that flips between float32 and float64 is no kernel error)


def make_net(ns, nc, hidden, act, passthrough, seed, dtype=torch.float32):
    """The package's NNDynamics with seeded weights (nn.Linear's own initialisation)."""
    from mpc.dynamics import NNDynamics
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        return NNDynamics(ns, nc, list(hidden), activation=act, passthrough=passthrough).to(dtype)
    finally:
        torch.random.set_rng_state(state)


def net_params(dx):
    return [layer.weight for layer in dx.fcs], [layer.bias for layer in dx.fcs]


def _slopes(a, act):
    if act == "sigmoid":
        s = a * (1. - a)
        return s, s * (1. - 2. * a)
    assert act == "relu"
    return (a > 0).to(a.dtype), torch.zeros_like(a)


def hidden_preactivations(Ws, bs, act, x, u):
    """[N, all hidden units] of h_l = W_l a_{l-1} + b_l in float64."""
    Ws, bs = [W.detach().to(F64) for W in Ws], [b.detach().to(F64) for b in bs]
    a, hs = torch.cat((x.detach().to(F64), u.detach().to(F64)), 1), []
    for W, b in zip(Ws[:-1], bs[:-1]):
        h = a @ W.T + b
        hs.append(h)
        a = torch.sigmoid(h) if act == "sigmoid" else torch.relu(h)
    return torch.cat(hs, 1) if hs else a.new_zeros(a.shape[0], 0)


def yardstick(Ws, bs, act, passthrough, x, u, gF, gf, chunk=1024):
    """float64 (F, f, grads, scales) at the points x [N,ns], u [N,nc] for cotangents gF [N,ns,n], gf [N,ns]; grads and scales
    are lists [W_1, b_1, ..., W_L, b_L] in nn.Linear's layouts."""
    Ws, bs = [W.detach().to(F64) for W in Ws], [b.detach().to(F64) for b in bs]
    x, u, gF, gf = (t.detach().to(F64) for t in (x, u, gF, gf))
    L, N, ns = len(Ws), x.shape[0], x.shape[1]
    n = ns + u.shape[1]
    grads = [torch.zeros_like(t) for pair in zip(Ws, bs) for t in pair]
    scales = [torch.zeros_like(t) for t in grads]
    Fs, fs = [], []
    for lo in range(0, max(N, 1), chunk):
        sl = slice(lo, min(N, lo + chunk))
        tau = torch.cat((x[sl], u[sl]), 1)
        m = tau.shape[0]
        a, s, d2, M, P = [tau], [None], [None], [None], [torch.eye(n, dtype=F64).expand(m, n, n)]
        for l in range(1, L):
            h = a[-1] @ Ws[l - 1].T + bs[l - 1]
            a.append(torch.sigmoid(h) if act == "sigmoid" else torch.relu(h))
            sl_, d2_ = _slopes(a[-1], act)
            s.append(sl_)
            d2.append(d2_)
            M.append(torch.matmul(Ws[l - 1], P[-1]))
            P.append(s[-1].unsqueeze(2) * M[-1])
        out = a[-1] @ Ws[-1].T + bs[-1]
        Fm = torch.matmul(Ws[-1], P[-1])
        if passthrough:
            out = out + x[sl]
            Fm = Fm + torch.eye(ns, n, dtype=F64)
        Fs.append(Fm)
        fs.append(out - (Fm * tau.unsqueeze(1)).sum(2))
        ch, cM = gf[sl], gF[sl] - gf[sl].unsqueeze(2) * tau.unsqueeze(1)
        for l in range(L, 0, -1):
            cW = cM @ P[l - 1].transpose(1, 2) + ch.unsqueeze(2) * a[l - 1].unsqueeze(1)
            grads[2 * l - 2] += cW.sum(0)
            scales[2 * l - 2] += cW.abs().sum(0)
            grads[2 * l - 1] += ch.sum(0)
            scales[2 * l - 1] += ch.abs().sum(0)
            if l > 1:
                cP = torch.matmul(Ws[l - 1].T, cM)
                ca = ch @ Ws[l - 1]
                cs = (cP * M[l - 1]).sum(2)
                ch = s[l - 1] * ca + d2[l - 1] * cs
                cM = s[l - 1].unsqueeze(2) * cP
    return torch.cat(Fs), torch.cat(fs), grads, scales


def module_autograd(dx, x, u, gF, gf):
    """d (sum gF F + sum gf f) / d (weights, biases) by float64 autograd through the package's NNDynamics.forward + grad_input
    (x, u detached leaves, as MPC.linearize_dynamics hands them in): (F, f, [gW_1, gb_1, ...])."""
    with torch.enable_grad():
        xt, ut = x.detach().clone().requires_grad_(True), u.detach().clone().requires_grad_(True)
        new_x = dx(xt, ut)
        R, S = dx.grad_input(xt, ut)
        Fm = torch.cat((R, S), 2)
        f = new_x - (R * xt.unsqueeze(1)).sum(2) - (S * ut.unsqueeze(1)).sum(2)
        Ws, bs = net_params(dx)
        params = [t for pair in zip(Ws, bs) for t in pair]
        g = torch.autograd.grad((gF * Fm).sum() + (gf * f).sum(), params, allow_unused=True)
    return Fm.detach(), f.detach(), [torch.zeros_like(p) if gi is None else gi for gi, p in zip(g, params)]


def random_points(Ws, bs, act, N, seed, dtype=torch.float32):
    """(x, u, gF, gf, rejected fraction): N standard-normal points in `dtype`.  For relu they are drawn by rejection on the
    float64 forward pass at the rounded inputs: a point is kept only if every hidden pre-activation has |h| >= REL_H."""
    g = torch.Generator().manual_seed(seed)
    n, ns = Ws[0].shape[1], Ws[-1].shape[0]
    # (at least 256 draws: the rejected fraction, which the callers hold to a quarter, is then a rate and not the luck of ten draws)
    M = N if act != "relu" or len(Ws) == 1 else max(int(math.ceil(1.5 * N)) + 8, 256)
    tau = torch.randn(M, n, generator=g, dtype=F64).to(dtype)
    x, u = tau[:, :ns], tau[:, ns:]
    keep = torch.ones(M, dtype=torch.bool)
    if M != N:
        keep = (hidden_preactivations(Ws, bs, act, x, u).abs() >= REL_H).all(1)
    rejected = 1. - float(keep.sum()) / M
    assert int(keep.sum()) >= N, "rejection left %d of %d points, %d wanted" % (int(keep.sum()), M, N)
    idx = keep.nonzero()[:N, 0]
    x, u = x[idx].contiguous(), u[idx].contiguous()
    gF = torch.randn(N, ns, n, generator=g, dtype=F64).to(dtype)
    gf = torch.randn(N, ns, generator=g, dtype=F64).to(dtype)
    return x, u, gF, gf, rejected


def check(got, grads, scales, rel=1e-3, ab=1e-4):
    """max over all entries of |err_k| / (rel |g_k| + ab scale_k) -- at most 1 within the limit."""
    worst = 0.
    for a, g, s in zip(got, grads, scales):
        lim = rel * g.abs() + ab * s
        err = (a.detach().cpu().to(F64) - g).abs()
        assert torch.isfinite(err).all()
        ratio = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        worst = max(worst, float(ratio.max()) if ratio.numel() else 0.)
    return worst
