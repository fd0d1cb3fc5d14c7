"""CPU: tests/strided_views.py itself -- the views show the values, carry the table's strides, leave NaN everywhere else in their
arena, and mpc._native._block_strided hands them to the C ABI as they are (no copy, the strides unchanged)."""
import numpy as np
import pytest
import torch

import strided_views as SV

T, B = 5, 3
INNERS = {"C": (16, 16), "c": (16,), "F": (12, 16), "f": (12,), "c_odd": (10,), "F_odd": (7, 10)}


def table(layout, blk, itemsize, pad=1):
    """The issue's table, written out once more: (st, sb, offset of the first block behind the 64 leading NaNs)."""
    g = 16 // itemsize
    up = (blk + g - 1) // g * g
    return {"dense": (B * blk, blk, 0), "shared": (0, 0, 0), "shared_b": (blk, 0, 0), "shared_t": (0, blk, 0),
            "batch_major": (blk, T * blk, 0), "slice_b": ((B + 3) * blk, blk, blk),
            "pitch_grid": (B * (up + g * pad) + 2 * g * pad, up + g * pad, 0), "pitch_off": (B * (blk + 1) + 1, blk + 1, 0)}[layout]


def values(inner, dtype):
    return np.random.default_rng(len(inner)).standard_normal((T, B) + inner).astype(dtype)


def expected(v, layout):
    return {"shared": np.broadcast_to(v[:1, :1], v.shape), "shared_b": np.broadcast_to(v[:, :1], v.shape),
            "shared_t": np.broadcast_to(v[:1], v.shape)}.get(layout, v)


@pytest.mark.parametrize("lib", [np, torch], ids=["numpy", "torch"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", SV.SINGLE)
@pytest.mark.parametrize("role", sorted(INNERS))
def test_a_placed_view_shows_the_values_through_the_tables_strides_in_an_arena_of_nan(role, layout, dtype, lib):
    inner = INNERS[role]
    blk = int(np.prod(inner))
    v = values(inner, dtype)
    for pad in (1, 2) if layout == "pitch_grid" else (1,):
        pl = SV.place(v, (layout, pad), lib)
        isz = np.dtype(dtype).itemsize
        st, sb, off = table(layout, blk, isz, pad)
        as_np = (lambda a: a.numpy()) if lib is torch else (lambda a: a)
        view, arena, dense = as_np(pl.view), as_np(pl.arena), as_np(pl.dense)
        assert view.shape == v.shape and np.array_equal(view, expected(v, layout)) and np.array_equal(dense, expected(v, layout))
        assert dense.flags["C_CONTIGUOUS"] and (pl.st, pl.sb) == (st, sb)
        inner_strides = tuple(int(np.prod(inner[i + 1:])) for i in range(len(inner)))
        assert tuple(s // isz for s in view.strides) == (st, sb) + inner_strides
        first = (view.ctypes.data - arena.ctypes.data) // isz
        assert first == SV.FRONT + off and SV.FRONT >= 64
        # everything the view does not show is NaN: in front, in every gap, and one T-stride plus 64 elements behind the last block
        seen = np.zeros(arena.size, bool)
        for t in range(T):
            for b in range(B):
                seen[first + t * st + b * sb:first + t * st + b * sb + blk] = True
        assert np.isnan(arena[~seen]).all() and not np.isnan(arena[seen]).any()
        last = np.flatnonzero(seen)[-1]
        assert arena.size - 1 - last >= st + 64 and np.flatnonzero(seen)[0] >= 64
        if layout in ("pitch_grid", "pitch_off", "slice_b"):
            assert (~seen[first:last]).any()          # there ARE gaps between the blocks
        if lib is np:
            assert view.ctypes.data % 16 == (off * isz) % 16
        if layout == "pitch_grid":
            assert st % (16 // isz) == 0 and sb % (16 // isz) == 0 and sb >= blk + 16 // isz
        if layout == "pitch_off":
            assert (sb * isz) % 16          # (st = B sb + 1 lands on the grid again where B + 1 is a multiple of g)


def test_the_mixed_layouts_give_every_tensor_a_pair_of_its_own():
    for layout, want in (("mixed_a", dict(C="batch_major", c="pitch_grid", F="slice_b", f="shared_b", qp_start=("pitch_grid", 2))),
                         ("mixed_b", dict(C="shared_b", c="slice_b", F="pitch_grid", f="batch_major", qp_start="batch_major"))):
        assert {role: SV.of(layout, role) for role in want} == want
        v = {role: values(INNERS[role], np.float32) for role in "CcFf"}
        qp = values((4,), np.float32)
        pl = SV.place_problem(layout, np, v["C"], v["c"], v["F"], v["f"], qp)
        pairs = [(pl[r].st, pl[r].sb) for r in ("C", "c", "F", "f", "qp_start")]
        assert len(set(pairs)) == 5, pairs
        for role, single in want.items():
            name, pad = single if isinstance(single, tuple) else (single, 1)
            blk = int(np.prod(pl[role].view.shape[2:]))
            assert (pl[role].st, pl[role].sb) == table(name, blk, 4, pad)[:2]
        assert SV.on_grid(pl, 4)
    # qp_start never shares the layout of the other four
    for layout in SV.SINGLE:
        assert SV.of(layout, "qp_start") != layout
    assert SV.GRID == tuple(l for l in SV.LAYOUTS if l != "pitch_off") and len(SV.LAYOUTS) == 10


@pytest.mark.parametrize("layout", SV.SINGLE)
def test_block_strided_hands_the_views_strides_through_and_does_not_copy(layout):
    from mpc import _native
    for role, inner_dims in (("C", 2), ("c", 1), ("F", 2), ("f", 1), ("c_odd", 1), ("F_odd", 2)):
        pl = SV.place(values(INNERS[role], np.float32), layout, torch)
        t, st, sb = _native._block_strided(pl.view, inner_dims)
        assert t.data_ptr() == pl.view.data_ptr() and t.stride() == pl.view.stride() and (st, sb) == (pl.st, pl.sb)
    # the whole problem struct: pointers and all eight strides are the views'
    v = {role: values(INNERS[role], np.float32) for role in "CcFf"}
    pl = SV.place_problem("mixed_a" if layout == "dense" else layout, torch, v["C"], v["c"], v["F"][:-1], v["f"][:-1])
    # (host tensors: _problem only reads pointers and strides)
    p, _keep = _native.HipBackend._problem(torch.zeros(B, 12), pl["C"].view, pl["c"].view, pl["F"].view, pl["f"].view, None, None)
    for role in "CcFf":
        assert getattr(p, role) == pl[role].view.data_ptr()
        assert (getattr(p, role + "_st"), getattr(p, role + "_sb")) == (pl[role].st, pl[role].sb)
