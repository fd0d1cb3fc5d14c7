"""TEST INFRASTRUCTURE shared by tests/test_emu_unvouched.py (CPU emulator) and tests/test_gpu_unvouched.py (device): the batches
a bare LQRStep call may bring that MPC.forward never does -- a nominal whose current_x is not the rollout of current_u from
x_init, and problems whose data is not finite -- with the float64 oracle's answer to each.

The reference starts its forward pass from new_x = [x_init], dx = [zeros_like(x_init)] (mpc/lqr_step.py:181-182): dx_0 = 0 and
new_x[0] = x_init whatever current_x[0] holds; old_cost is the cost of the nominal as given (:169)."""
import numpy as np

MODES = ("free", "box", "tbox", "delta", "mask")       # unbounded, scalar box, tensor box, delta_u, u_zero_I
KINDS = ("ok", "x0_big", "x0_small", "both")
OUTPUTS = ("new_x", "new_u", "costs", "old_costs", "alphas", "full_du_norm", "alpha_du_norm", "K", "k")


def kinds_of(B, rot=0):
    """Which kind of nominal each problem of a batch of B gets.
    B = 9 (four problems per wavefront: the 12/4 kernels and the row-per-problem kernel): in-wave positions 0 and 3 of the first wave
            and the tail wave's only problem (three idle rows beside it) are special, the second wave is full and healthy;
    B = 70 (a lane per problem): lanes 0 and 63 of the first wave, lane 0 of the second;
    B = 3 (a wavefront per problem -- mfma16 and the 32/8 family -- no wave-mates): three of the four kinds, rotated by `rot`."""
    kinds = ["ok"] * B
    if B == 9:
        kinds[0], kinds[3], kinds[8] = "x0_big", "x0_small", "both"
    elif B == 70:
        kinds[0], kinds[63], kinds[64] = "x0_big", "x0_small", "both"
    else:
        assert B == 3
        kinds = [("x0_big", "x0_small", "both", "ok")[(rot + i) % 4] for i in range(3)]
    return kinds


def make_batch(seed, ns, nc, T, B, mode, with_f=True, kinds=None, dtype=np.float32):
    """A random convex batch (the recipe of the emulator tests' _pad_problem / _ns_problem) whose nominal is the rollout of
    cur_u from x_init, then moved off it per `kinds`:
      x0_big / x0_small: x_init += 0.5 / 1e-3 (current_x untouched, so current_x[0] != x_init);
      both             : current_x[2:] += 0.05 N(0,1) and x_init += 0.5.
    Rounded to `dtype` (what the kernel reads); the oracle gets the same numbers in float64.  -> (kw, off [B] bool)"""
    from oracle import lqr_oracle as O
    rng = np.random.default_rng(seed)
    n = ns + nc
    A = rng.standard_normal((T, B, n, n))
    C = np.einsum("tbji,tbjk->tbik", A, A) + 0.1 * np.eye(n)
    c = rng.standard_normal((T, B, n))
    F = np.concatenate((np.eye(ns) + 0.2 * rng.standard_normal((max(T - 1, 0), B, ns, ns)) / np.sqrt(ns),
                        rng.standard_normal((max(T - 1, 0), B, ns, nc)) / np.sqrt(ns)), 3)
    f = 0.1 * rng.standard_normal((max(T - 1, 0), B, ns)) if with_f else None
    x_init = rng.standard_normal((B, ns))
    cur_u = np.clip(0.3 * rng.standard_normal((T, B, nc)), -0.4, 0.4)
    lo_t, hi_t = -0.5 - rng.random((T, B, nc)), 0.5 + rng.random((T, B, nc))
    mask = rng.random((T, B, nc)) < 0.35
    shift = 0.05 * rng.standard_normal((T, B, ns))
    rd = lambda a: None if a is None else np.ascontiguousarray(a, dtype).astype(np.float64)
    C, c, F, f, x_init, cur_u, lo_t, hi_t = map(rd, (C, c, F, f, x_init, cur_u, lo_t, hi_t))
    cur_x = rd(O.traj_cost(x_init, cur_u, F, f)[0])
    # (the rounded rollout obeys the rounded dynamics to float32 rounding: inside the kernels' 1e-5 (1 + |x|) test)
    off = np.zeros(B, bool)
    for b, kind in enumerate(kinds or ["ok"] * B):
        if kind == "ok":
            continue
        off[b] = True
        x_init[b] = rd(x_init[b] + (1e-3 if kind == "x0_small" else 0.5))
        if kind == "both" and T > 2:
            cur_x[2:, b] = rd(cur_x[2:, b] + shift[2:, b])
    kw = dict(x_init=x_init, C=C, c=c, F=F, f=f, cur_x=cur_x, cur_u=cur_u)
    if mode == "box":
        kw.update(u_lower=-0.5, u_upper=0.5)
    elif mode == "tbox":
        kw.update(u_lower=lo_t, u_upper=hi_t)
    elif mode == "delta":
        kw.update(u_lower=-0.5, u_upper=0.5, delta_u=0.1)
    elif mode == "mask":
        kw.update(u_zero_I=mask)
    else:
        assert mode == "free"
    return kw, off


def oracle(kw, keep=None):
    """The float64 oracle, one reference call per problem (lockstep=False), gains included; `keep`: on those problems alone."""
    from oracle import lqr_oracle as O
    if keep is not None:
        kw = take(kw, keep)
    return O.lqr_step(lockstep=False, return_gains=True, **kw)


def take(kw, keep):
    """The problems `keep` [B] bool of a batch's keyword arguments."""
    out = {}
    for k, v in kw.items():
        if isinstance(v, np.ndarray) and v.ndim >= 3:
            v = v[:, keep]
        elif isinstance(v, np.ndarray) and v.ndim == 2:
            v = v[keep]
        out[k] = v
    return out


def sel(r, key, keep):
    """Output `key` of a result restricted to the problems `keep`."""
    v = np.asarray(r[key])
    return v[keep] if v.ndim == 1 else v[:, keep]


POISONS = ("nan_c", "nan_C", "nan_u", "inf_x0", "overflow_F", "nan_bound", "nan_f")


def poison(kw, name, who, big=1e30):
    """A copy of the batch with the problems `who` made non-finite: NaN in c, C, cur_u, a tensor bound or f; +inf in x_init; F scaled
    by `big` per step, until the rollout overflows the kernel's number format (1e30 passes float32 in two steps; a float64 caller
    gives 1e200)."""
    kw = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    T = kw["C"].shape[0]
    for b in who:
        if name == "nan_c":
            kw["c"][T // 2, b, 1 % kw["c"].shape[2]] = np.nan
        elif name == "nan_C":
            kw["C"][T // 2, b, 0, 0] = np.nan
        elif name == "nan_u":
            kw["cur_u"][T // 2, b, 0] = np.nan
        elif name == "inf_x0":
            kw["x_init"][b, 0] = np.inf
        elif name == "overflow_F":
            kw["F"][:, b] *= big
        elif name == "nan_bound":
            kw["u_upper"][T // 2, b, 0] = np.nan
        elif name == "nan_f":
            kw["f"][T // 2, b, 0] = np.nan
        else:
            raise KeyError(name)
    return kw


def rot_of(mode, T, with_f):
    """the rotation kinds_of gives a batch of three in this case (every kind meets every mode somewhere)"""
    return MODES.index(mode) + (1 if T == 1 else 0) + (2 if not with_f else 0)


# The inputs that come back FINITE and UNFLAGGED, by name (kernel family, mode, poison) -- the same list stands in INTEGRATION.md
# under the status word.  Anything else non-finite in a problem's data sets MPC_ST_NONFINITE on that problem.
#   * the box clamp absorbs a NaN nominal control: eclampf(NaN, lo, hi) returns a bound on the 32/8 family (its clamp is max/min,
#     which drop a NaN operand), where the reference's util.eclamp keeps the NaN.  Changing the clamp is not part of this file.
#   * a NaN in a tensor bound never binds, on any kernel: every comparison with it is false, in the box QP and in the rollout's
#     clamp alike, and that control is simply unbounded on that side at that timestep.  (The reference's util.eclamp assigns a bound
#     only where x < lower / x > upper holds, so its rollout does the same.)
FINITE_AND_UNFLAGGED = {
    ("m40", "box", "nan_u"), ("pad", "box", "nan_u"),
} | {(fam, "tbox", "nan_bound") for fam in ("dpp", "m16", "m16_f64", "tiny_f32", "tiny_f64", "wave1", "m40", "pad")}


def special_problems(B):
    return [0, 3, 8] if B == 9 else ([0, 63, 64] if B == 70 else [1])


POISON_CASES = [("free", p) for p in ("nan_c", "nan_C", "nan_u", "inf_x0", "overflow_F", "nan_f")] + \
               [("box", p) for p in ("nan_c", "nan_C", "nan_u", "inf_x0", "overflow_F", "nan_f")] + [("tbox", "nan_bound")]
