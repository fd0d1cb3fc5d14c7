"""CPU-only, no launch: the support rules of csrc/lqr_rules.hip and the route entries, ONE stride (or one base pointer) at a time.

tests/golden/make_golden_step_route.py skews every stride at once, so a rule that forgot one of them passes there.  Here an aligned
float32 problem over made-up addresses has one of C_st, C_sb, c_st, c_sb, F_st, F_sb, f_st, f_sb moved by one element, or one of its
base pointers by 4 bytes (tests/stride_rules_probe.cpp, built host-only against the library under test), and

  * every rule answers what NEEDS below says -- written by hand from the kernels: which of the caller's blocks each one fetches in
    16-byte granules (lqr_dpp16_body.h: C, c, F, f and the nominal by LDS-DMA; lqr_mfma40_body.h: the same and x_init; the padded
    instantiations' 16-byte gathers: C and F alone, c, f and the nominal ride as dwords; the KKT kernels read no f);
  * no route entry picks a kernel whose rule asks for the moved alignment: a forced exact kernel is refused with MPC_E_DIMS, impl 0 /
    kernel 0 fall to the padded instantiation -- with dword gathers where C or F moved --, the gradient route to the wavefront kernels.

mpc_lqr_impl_supported answers the same way for the two exact kernels: 1 on the grid, 0 once a block the kernel streams in 16-byte
granules has its base or a stride off it (it looks at the blocks the problem names; a query by sizes alone names none).
The 16-byte form of kkt_wave64 is chosen inside its launcher (kkt_wave64.hip: wave64_aligned, not exported): its choice shows on the
device alone: tests/test_gpu_strided.py runs the 16-byte form under its grid layouts and the dword form under pitch_off, each against a
dense control that takes the same form."""
import json
import os
import subprocess

import pytest

from conftest import ROOT
from mpc import _native

E_DIMS = -1
STRIDES = ("C_st", "C_sb", "c_st", "c_sb", "F_st", "F_sb", "f_st", "f_sb")
POINTERS = ("C", "c", "F", "f", "x_init", "cur_x", "cur_u")
MOVES = [None] + list(STRIDES) + list(POINTERS)

CcF = {"C", "C_st", "C_sb", "c", "c_st", "c_sb", "F", "F_st", "F_sb"}
NEEDS = {
    # the step kernels
    "dpp16": CcF | {"f", "f_st", "f_sb", "cur_x", "cur_u"},
    "mfma40": CcF | {"f", "f_st", "f_sb", "cur_x", "cur_u", "x_init"},
    "mfma40_pad16": {"C", "C_st", "C_sb", "F", "F_st", "F_sb"},
    "dpp16_pad": set(), "mfma40_pad": set(), "mfma40_narrow": set(),
    # the KKT backward: gradients alone, and fused
    "kkt_dpp16": CcF | {"cur_x", "cur_u"},
    "kkt_fused_dpp16": CcF | {"cur_x", "cur_u"},
    "kkt_fused_mfma40": CcF | {"cur_x", "cur_u"},
    "kkt_fused_mfma40_pad16": {"C", "C_st", "C_sb", "F", "F_st", "F_sb"},
    "kkt_fused_mfma40_narrow16": {"C", "C_st", "C_sb", "F", "F_st", "F_sb"},
    "kkt_fused_dpp16_pad": set(), "kkt_fused_mfma40_pad": set(), "kkt_fused_mfma40_narrow": set(),
}
# which rules take the SHAPE at all
SHAPES = {
    (12, 4): {"dpp16", "dpp16_pad", "mfma40_pad", "mfma40_pad16", "mfma40_narrow", "kkt_dpp16", "kkt_fused_dpp16", "kkt_fused_dpp16_pad",
              "kkt_fused_mfma40_pad", "kkt_fused_mfma40_pad16", "kkt_fused_mfma40_narrow", "kkt_fused_mfma40_narrow16"},
    (32, 8): {"mfma40", "mfma40_pad", "mfma40_pad16", "kkt_fused_mfma40", "kkt_fused_mfma40_pad", "kkt_fused_mfma40_pad16"},
    (16, 4): {"mfma40_pad", "mfma40_pad16", "mfma40_narrow", "kkt_fused_mfma40_pad", "kkt_fused_mfma40_pad16", "kkt_fused_mfma40_narrow",
              "kkt_fused_mfma40_narrow16"},
    (24, 8): {"mfma40_pad", "mfma40_pad16", "kkt_fused_mfma40_pad", "kkt_fused_mfma40_pad16"},
}
T, B = 5, 3
KKT_DPP16, KKT_DPP16_PAD, KKT_MFMA40, KKT_PAD16, KKT_PAD4, KKT_NARROW16, KKT_NARROW4, KKT_PREFER_NARROW = 1, 2, 3, 4, 5, 6, 7, 100
GRADS_DPP16, GRADS_WAVE = 1, 2


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    _native.load()
    exe = str(tmp_path_factory.mktemp("probe") / "stride_rules_probe")
    lib_dir = os.path.dirname(os.path.abspath(_native.lib_path()))
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-x", "hip", "--cuda-host-only",
                           os.path.join(ROOT, "tests", "stride_rules_probe.cpp"), "-o", exe, "-L" + lib_dir, "-lmpc_lqr_hip",
                           "-Wl,-rpath," + lib_dir])

    def run(calls):
        env = {k: v for k, v in os.environ.items() if k not in ("MPC_DPP16_RING", "MPC_MFMA40_RING", "MPC_DPP16_RESIDENT")}
        text = "".join(" ".join(str(v) for v in c) + "\n" for c in calls)
        out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, env=env, check=True).stdout.decode().splitlines()
        assert len(out) == len(calls)
        return [json.loads(line) for line in out]
    return run


def call(ns, nc, bounds, has_f, move):
    strides = [1 if move == s else 0 for s in STRIDES]
    pointers = [4 if move == q else 0 for q in POINTERS]
    return [ns, nc, T, B, bounds, int(has_f)] + strides + pointers


@pytest.fixture(scope="module")
def answers(probe):
    keys = [(shape, bounds, has_f, move) for shape in SHAPES for bounds in (0, 1) for has_f in (True, False) for move in MOVES
            if has_f or move not in ("f", "f_st", "f_sb")]
    got = probe([call(*shape, bounds, has_f, move) for shape, bounds, has_f, move in keys])
    return dict(zip(keys, got))


def moved(needs, move, has_f):
    return move is not None and move in needs and (has_f or move not in ("f", "f_st", "f_sb"))


def test_every_rule_asks_for_exactly_the_strides_and_pointers_its_kernel_moves_16_bytes_through(answers):
    for (shape, bounds, has_f, move), got in answers.items():
        for rule, needs in NEEDS.items():
            want = rule in SHAPES[shape] and not moved(needs, move, has_f)
            assert got["rules"][rule] == int(want), (shape, bounds, has_f, move, rule)
    # the table means something: every stride and every pointer refuses at least the two exact step kernels' union
    assert set(STRIDES) | set(POINTERS) == NEEDS["mfma40"] and NEEDS["dpp16"] == NEEDS["mfma40"] - {"x_init"}


def test_the_step_route_never_picks_a_kernel_that_asks_for_the_moved_alignment(answers):
    for (shape, bounds, has_f, move), got in answers.items():
        step = {int(k): dict(zip(("code", "kernel", "pad16", "entry", "query"), v)) for k, v in got["step"].items()}
        gathers = not moved(NEEDS["mfma40_pad16"], move, has_f)
        where = (shape, bounds, has_f, move)
        if shape == (12, 4):
            exact = not moved(NEEDS["dpp16"], move, has_f)
            assert (step[3]["code"], step[3]["entry"]) == ((0, 3) if exact else (E_DIMS, E_DIMS)), where
            assert step[3]["query"] == int(exact), where
            assert (step[0]["code"], step[0]["kernel"], step[0]["entry"]) == (0, 3 if exact else 8, 3 if exact else 8), where
            assert (step[8]["code"], step[8]["kernel"], step[8]["query"]) == (0, 8, 1), where    # the padded one takes every move
            assert step[5]["entry"] == E_DIMS
        elif shape == (32, 8):
            exact = not moved(NEEDS["mfma40"], move, has_f)
            assert (step[5]["code"], step[5]["entry"]) == ((0, 5) if exact else (E_DIMS, E_DIMS)), where
            assert step[5]["query"] == int(exact), where
            assert (step[0]["code"], step[0]["kernel"], step[0]["entry"]) == (0, 5 if exact else 7, 5 if exact else 7), where
            if not exact:
                assert step[0]["pad16"] == int(gathers), where
            assert (step[7]["code"], step[7]["kernel"], step[7]["pad16"], step[7]["query"]) == (0, 7, int(gathers), 1), where
            assert step[3]["entry"] == E_DIMS and step[9]["entry"] == E_DIMS
        else:
            # 16/4 and 24/8: impl 0 and a forced 7 on the padded kernel, a forced 9 on one state tile at 16/4; 16-byte gathers
            # only while C and F stay on the grid
            for impl in (0, 7) + ((9,) if shape == (16, 4) else ()):
                assert (step[impl]["code"], step[impl]["kernel"], step[impl]["pad16"]) == (0, impl or 7, int(gathers)), where + (impl,)
                assert step[impl]["entry"] == (impl or 7)
            assert step[3]["entry"] == E_DIMS and step[5]["entry"] == E_DIMS


def test_the_kkt_routes_never_pick_a_kernel_that_asks_for_the_moved_alignment(answers):
    for (shape, bounds, has_f, move), got in answers.items():
        kkt = {int(k): v for k, v in got["kkt"].items()}
        where = (shape, bounds, has_f, move)
        gathers = not moved(NEEDS["kkt_fused_mfma40_pad16"], move, has_f)
        if shape == (12, 4):
            exact = not moved(NEEDS["kkt_fused_dpp16"], move, has_f)
            assert kkt[KKT_DPP16] == (KKT_DPP16 if exact else E_DIMS), where
            assert kkt[0] == (KKT_DPP16 if exact else KKT_DPP16_PAD), where
            assert kkt[KKT_DPP16_PAD] == KKT_DPP16_PAD and kkt[KKT_PREFER_NARROW] == kkt[0], where
            assert got["grads"] == (GRADS_DPP16 if not moved(NEEDS["kkt_dpp16"], move, has_f) else GRADS_WAVE), where
        elif shape == (32, 8):
            exact = not moved(NEEDS["kkt_fused_mfma40"], move, has_f)
            assert kkt[KKT_MFMA40] == (KKT_MFMA40 if exact else E_DIMS), where
            assert kkt[0] == (KKT_MFMA40 if exact else (KKT_PAD16 if gathers else KKT_PAD4)), where
            assert got["grads"] == GRADS_WAVE
        else:
            assert kkt[0] == (KKT_PAD16 if gathers else KKT_PAD4), where
            assert got["grads"] == GRADS_WAVE
        if shape != (12, 4):
            assert kkt[KKT_PAD16] == (KKT_PAD16 if gathers else E_DIMS) and kkt[KKT_PAD4] == KKT_PAD4, where
        if shape == (16, 4):
            assert kkt[KKT_NARROW16] == (KKT_NARROW16 if gathers else E_DIMS) and kkt[KKT_NARROW4] == KKT_NARROW4, where
            assert kkt[KKT_PREFER_NARROW] == (KKT_NARROW16 if gathers else KKT_NARROW4), where
