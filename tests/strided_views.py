"""TEST INFRASTRUCTURE: the layouts in which C, c, F, f (and qp_start) reach the kernels as VIEWS -- include/mpc_lqr.h takes each
through its own element strides of the T and B axes, and mpc._native._block_strided hands a tensor's strides through as they are.

place(values, layout, lib) carves a [T, B, *inner] view holding `values` out of one arena pre-filled with NaN: at least 64 NaNs in
front of the first block, one T-stride plus 64 behind the last, NaN in every gap.  A kernel that reads a neighbour's or a gap's
element and uses it shows as NaN (or a wrong number) in an output.  lib is numpy or torch, so that the emulator tests and the GPU
tests share one definition.  blk = prod(inner), g = elements in 16 bytes:

    dense        st = B blk,        sb = blk            the control
    shared       0, 0                                    .expand(T, B, ...) of one block           (values: block [0, 0])
    shared_b     blk, 0                                  a [T, ...] tensor expanded over the batch (values: problem 0)
    shared_t     0, blk                                  a [B, ...] tensor expanded over time      (values: timestep 0)
    batch_major  blk, T blk                              storage [B, T, ...] through transpose(0, 1): st < sb
    slice_b      (B + 3) blk, blk, base + blk            [:, 1:1 + B] of a batch of B + 3
    pitch_grid   B sb + 2 g pad, sb = blk rounded up to g, + g pad       pitched, everything on the 16-byte grid
    pitch_off    B sb + 1, sb = blk + 1                  pitched, off the grid (float32: 4 bytes off)
    mixed_a      C batch_major, c pitch_grid, F slice_b, f shared_b, qp_start pitch_grid with pad = 2
    mixed_b      C shared_b, c slice_b, F pitch_grid, f batch_major, qp_start batch_major

Under any other layout qp_start is dense when C, c, F, f are not, and batch_major when they are: a layout of its own every time.
"""
import collections

import numpy as np

FRONT = 64
SINGLE = ("dense", "shared", "shared_b", "shared_t", "batch_major", "slice_b", "pitch_grid", "pitch_off")
MIXED = {"mixed_a": dict(C="batch_major", c="pitch_grid", F="slice_b", f="shared_b", qp_start=("pitch_grid", 2)),
         "mixed_b": dict(C="shared_b", c="slice_b", F="pitch_grid", f="batch_major", qp_start="batch_major")}
LAYOUTS = SINGLE + tuple(MIXED)
GRID = tuple(l for l in LAYOUTS if l != "pitch_off")        # every stride and every base on 16 bytes (blk a multiple of g)
SLICE_B0, SLICE_EXTRA = 1, 3

Placed = collections.namedtuple("Placed", "view dense arena st sb")


def of(layout, role):
    """The single layout (or (layout, pad)) of one tensor -- role in C, c, F, f, qp_start -- under a layout of the table."""
    if layout in MIXED:
        return MIXED[layout][role]
    if role == "qp_start":
        return "batch_major" if layout == "dense" else "dense"
    return layout


def geometry(T, B, blk, layout, itemsize, pad=1):
    """-> (st, sb, base, arena elements): strides and the first block's offset in elements, FRONT included."""
    g = 16 // itemsize
    if layout == "dense":
        st, sb, base = B * blk, blk, 0
    elif layout == "shared":
        st, sb, base = 0, 0, 0
    elif layout == "shared_b":
        st, sb, base = blk, 0, 0
    elif layout == "shared_t":
        st, sb, base = 0, blk, 0
    elif layout == "batch_major":
        st, sb, base = blk, T * blk, 0
    elif layout == "slice_b":
        st, sb, base = (B + SLICE_EXTRA) * blk, blk, SLICE_B0 * blk
    elif layout == "pitch_grid":
        sb = -(-blk // g) * g + g * pad
        st, base = B * sb + 2 * g * pad, 0
    elif layout == "pitch_off":
        sb = blk + 1
        st, base = B * sb + 1, 0
    else:
        raise KeyError(layout)
    extent = base + (T - 1) * st + (B - 1) * sb + blk
    return st, sb, FRONT + base, FRONT + extent + st + 64


def _is_torch(lib):
    return lib.__name__ == "torch"


def place(values, layout, lib, pad=1, device=None):
    """values [T, B, *inner] (numpy) -> Placed(view, dense, arena, st, sb): the view of the arena under `layout` (a single one, or
    (layout, pad)), the dense [T, B, *inner] array of exactly the numbers the view shows, the arena itself, and the two strides in
    elements.  torch: the arena lives on `device`."""
    if isinstance(layout, tuple):
        layout, pad = layout
    values = np.asarray(values)
    T, B = values.shape[:2]
    inner = tuple(values.shape[2:])
    blk = int(np.prod(inner)) if inner else 1
    if layout == "shared":
        shown = np.broadcast_to(values[:1, :1], values.shape)
    elif layout == "shared_b":
        shown = np.broadcast_to(values[:, :1], values.shape)
    elif layout == "shared_t":
        shown = np.broadcast_to(values[:1], values.shape)
    else:
        shown = values
    shown = np.ascontiguousarray(shown)
    st, sb, base, total = geometry(T, B, blk, layout, values.dtype.itemsize, pad)
    # the arena's first element on 64 bytes, whatever the allocator gave (numpy promises 16 at the most)
    raw = np.full(total + 64, np.nan, values.dtype)
    skip = (-raw.ctypes.data % 64) // values.dtype.itemsize
    arena = raw[skip:skip + total]
    inner_strides = []
    acc = 1
    for d in reversed(inner):
        inner_strides.insert(0, acc)
        acc *= d
    isz = values.dtype.itemsize
    view = np.lib.stride_tricks.as_strided(arena[base:], values.shape, tuple(s * isz for s in (st, sb, *inner_strides)))
    # written block by block: under a shared layout the same block is written more than once, always with the same numbers
    for t in range(T):
        for b in range(B):
            view[t, b] = shown[t, b]
    if _is_torch(lib):
        t_arena = lib.from_numpy(np.ascontiguousarray(arena)).to(device)
        t_view = t_arena.as_strided(tuple(values.shape), (st, sb, *inner_strides), base)
        return Placed(t_view, lib.from_numpy(shown.copy()).to(device), t_arena, st, sb)
    return Placed(view, shown, arena, st, sb)


def place_problem(layout, lib, C, c, F=None, f=None, qp_start=None, device=None):
    """{role: Placed} of one problem's tensors under a layout of the table (None stays None)."""
    return {role: (None if v is None else place(v, of(layout, role), lib, device=device))
            for role, v in (("C", C), ("c", c), ("F", F), ("f", f), ("qp_start", qp_start))}


def on_grid(placed, itemsize):
    """Do the first block and both strides of every placed tensor lie on 16 bytes (what the exact 12/4 and 32/8 kernels ask for)?"""
    g = 16 // itemsize
    for p in placed.values():
        if p is None:
            continue
        ptr = p.view.data_ptr() if hasattr(p.view, "data_ptr") else p.view.ctypes.data
        if ptr % 16 or p.st % g or p.sb % g:
            return False
    return True


# ---- the cases the emulator and the device tests build on the placed values ----
def f64(a):
    return None if a is None else np.asarray(a, np.float64)


def cut(z, T, B=None):
    """The first T timesteps (and B problems) of a step fixture as step_kwargs, the nominal re-derived by O.traj_cost."""
    from helpers import step_kwargs
    kw = step_kwargs(z)
    B = kw["C"].shape[1] if B is None else B
    for k in ("C", "c", "cur_u", "u_zero_I", "u_lower", "u_upper"):
        if isinstance(kw.get(k), np.ndarray):
            kw[k] = kw[k][:T, :B]
    kw["F"] = kw["F"][:T - 1, :B]
    if kw.get("f") is not None:
        kw["f"] = kw["f"][:T - 1, :B]
    kw["x_init"] = kw["x_init"][:B]
    return renominal(kw)


def renominal(kw):
    from oracle import lqr_oracle as O
    dt = kw["C"].dtype
    kw["cur_x"] = O.traj_cost(f64(kw["x_init"]), f64(kw["cur_u"]), f64(kw["F"]), f64(kw.get("f")))[0].astype(dt)
    return kw


def random_case(ns, nc, T, B, seed, bounds=None, dtype=np.float32):
    """The recipe of tests/test_emu_mfma16.py's _pad_problem, rounded to the kernel's dtype before the nominal is rolled out."""
    rng = np.random.default_rng(seed)
    n = ns + nc
    A = rng.standard_normal((T, B, n, n))
    kw = dict(C=np.einsum("tbji,tbjk->tbik", A, A) + 0.1 * np.eye(n), c=rng.standard_normal((T, B, n)),
              F=np.concatenate((np.eye(ns) + 0.2 * rng.standard_normal((T - 1, B, ns, ns)) / np.sqrt(ns),
                                rng.standard_normal((T - 1, B, ns, nc)) / np.sqrt(ns)), 3),
              f=0.1 * rng.standard_normal((T - 1, B, ns)), x_init=rng.standard_normal((B, ns)),
              cur_u=np.clip(0.3 * rng.standard_normal((T, B, nc)), -0.4, 0.4))
    kw = {k: v.astype(dtype) for k, v in kw.items()}
    if bounds is not None:
        kw.update(u_lower=-bounds, u_upper=bounds)
    return renominal(kw)


def shown(kw, layout):
    """kw with C, c, F, f replaced by the dense arrays a view under `layout` shows; the nominal follows where F or f changed."""
    pl = place_problem(layout, np, kw["C"], kw["c"], kw["F"], kw.get("f"))
    d = dict(kw)
    for role in ("C", "c", "F", "f"):
        if pl[role] is not None:
            d[role] = pl[role].dense
    if any(of(layout, role) in ("shared", "shared_b", "shared_t") for role in ("F", "f")):
        d = renominal(d)
    return d
