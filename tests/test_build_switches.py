"""CPU-only, compiles nothing: every MPC_* name that a preprocessor conditional under csrc/ tests has a user that can be named.

Each name on an #if / #ifdef / #ifndef / #elif line is exactly one of
  (a) given as -DNAME on a compile line: csrc/Makefile's (`make -n -B`, as tests/test_makefile_flags.py reads them) or an emulator
      build line of tests/ (the "-DNAME..." words of the lists those builds hand their compiler -- the resident-F placement's two,
      the Makefile's RES_FLAGS, are given there),
  (b) #defined inside csrc/ or include/ outside a `#ifndef NAME` default of its own (a derived macro or an include guard),
  (c) listed in OTHER_USERS below next to the existing file that sets it.
A switch that nothing sets is an alternative nobody compiles: it is deleted with its branch (docs/history/r25.md), and REMOVED keeps
the names of that prune out of csrc/."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc.pytorch_amd", "csrc")

# (c) name -> the file that sets it (relative to the repository)
OTHER_USERS = {
    # diagnostic builds that scripts in tools/ still make (tools/build_variant.sh NAME -D...)
    "MPC_DPP16_PROF": "tools/prof_phases.py",
    "MPC_MFMA40_PROF": "tools/prof_phases40.py",
    "MPC_QP_START": "tools/README.md",
    # the host emulator's own definitions in front of the bodies it includes
    "MPC_STAT": "tests/emu/emu_mfma16.cpp",
    "MPC_DEVM": "tests/emu/emu_mfma16.cpp",
}

# the switches docs/history/r25.md deleted: none of them comes back under csrc/ in any role
REMOVED = """MPC_DPP16_QP_LDL MPC_DPP16_DPP_BCAST MPC_DPP16_KEEP_KM MPC_DPP16_NO_CPERM MPC_DPP16_PROBE_ROLL_F MPC_PAD_PROBE_DUP
MPC_DPP16_RSLOTS MPC_KF_SKIP MPC_DPP16_OUT_CACHED MPC_KF_CACHED_GRADS MPC_DPP16_C_AUX MPC_DPP16_FR_AUX MPC_KKT_LD_AUX
MPC_MFMA40_QP_LDL MPC_MFMA40_KPAD MPC_KF40_VFULL MPC_KF40_NOVS MPC_KF40_P1_ONLY MPC_KF40_NO_OUTER MPC_CFG5_SWEEP_ONLY MPC_MFMA40_C_AUX
MPC_W1_SKIP MPC_W1_PROF MPC_DPP16_RESIDENT_DEFAULT MPC_DPP16_QP_WARM MPC_MFMA16_QP_WARM MPC_MFMA40_QP_WARM""".split()

CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")
DIRECTIVE = re.compile(r"^\s*#\s*(if|ifdef|ifndef|else|elif|endif|define)\b\s*(\w*)")


def sources(*dirs):
    out = []
    for d in dirs:
        for pat in ("*.h", "*.hip", "*.hpp", "*.cpp"):
            out += glob.glob(os.path.join(ROOT, d, pat))
    return sorted(out)


def code_lines(path):
    """The file's lines with continuation lines joined and // comments cut off."""
    text = open(path, errors="replace").read().replace("\\\n", " ")
    return [l.split("//")[0] for l in text.split("\n")]


def names_tested():
    names = {}
    for path in sources("mpc.pytorch_amd/csrc"):
        for l in code_lines(path):
            m = CONDITIONAL.match(l)
            if m:
                for n in re.findall(r"\bMPC_\w+", m.group(2)):
                    names.setdefault(n, os.path.basename(path))
    return names


def defined_names():
    """Names #defined under csrc/ or include/ somewhere that is not the body of their own `#ifndef NAME`."""
    out = set()
    for path in sources("mpc.pytorch_amd/csrc", "include"):
        stack = []                                   # the name whose #ifndef default encloses the line, or None, per open conditional
        for l in code_lines(path):
            m = DIRECTIVE.match(l)
            if not m:
                continue
            kind, word = m.groups()
            if kind in ("if", "ifdef", "ifndef"):
                stack.append(word if kind == "ifndef" else None)
            elif kind in ("else", "elif"):
                stack[-1] = None
            elif kind == "endif":
                stack.pop()
            elif word.startswith("MPC_") and word not in stack:
                out.add(word)
        assert not stack, path
    return out


def compile_line_names():
    """-DNAME of the Makefile's compile commands and of the emulator builds in tests/."""
    out = set()
    if shutil.which("make"):
        text = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "--no-print-directory"]).decode()
        assert text.count(" -c ") >= 27, text
        out |= set(re.findall(r"\s-D(MPC_\w+)", text))
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        if os.path.basename(path) != os.path.basename(__file__):
            out |= set(re.findall(r"[\"']-D(MPC_\w+)", open(path).read()))
    return out


@pytest.mark.skipif(shutil.which("make") is None, reason="needs make")
def test_every_tested_switch_names_its_user():
    tested, on_lines, defined = names_tested(), compile_line_names(), defined_names()
    assert len(tested) >= 20, tested
    for name, where in sorted(tested.items()):
        roles = [r for r, yes in (("a compile line", name in on_lines), ("a #define in csrc/ or include/", name in defined),
                                  ("OTHER_USERS", name in OTHER_USERS)) if yes]
        assert len(roles) == 1, "%s (tested in %s): set by %s -- a switch has exactly one kind of user" % (name, where, roles or "nothing")
    for name, rel in sorted(OTHER_USERS.items()):
        assert name in tested, "%s is no longer tested under csrc/: drop it from OTHER_USERS" % name
        path = os.path.join(ROOT, rel)
        assert os.path.isfile(path), rel
        assert re.search(r"%s\b" % name, open(path, errors="replace").read()), "%s does not name %s" % (rel, name)          # (-DNAME too)


def test_the_pruned_switches_stay_out():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path) and not path.endswith((".o", ".so")):
            text = open(path, errors="replace").read()
            for name in REMOVED:
                assert not re.search(r"\b%s\b" % name, text), "%s is back in %s" % (name, os.path.basename(path))
