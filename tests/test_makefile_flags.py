"""CPU-only, compiles nothing: the flag lists that tools/isa_lint.py (FLAGS, SOURCES) and tests/test_isa_lint_dpp16_resident.py (BASE)
keep for their own compilations are the ones csrc/Makefile compiles the library's objects with.  `make -n -B <object>` prints the
command the Makefile would run; its -D... and -mllvm ... flags and its source are compared with those lists."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc.pytorch_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint                                  # noqa: E402
import test_isa_lint_dpp16_resident as res_lint   # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("make") is None, reason="needs make")


def compile_command(name):
    """(the -D / -mllvm flags, the source file) of the one command `make <name>.o` would run."""
    out = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "--no-print-directory", name + ".o"]).decode()
    lines = [l.split() for l in out.split("\n") if " -c " in l and l.split()[-2:] == ["-o", name + ".o"]]
    assert len(lines) == 1, out
    words, flags = lines[0], []
    for i, w in enumerate(words):
        if w.startswith("-D"):
            flags.append(w)
        elif w == "-mllvm":
            flags += [w, words[i + 1]]
    return flags, words[words.index("-c") + 1]


def flag_set(flags):
    """-mllvm and its argument are one flag."""
    it, out = iter(flags), []
    for w in it:
        out.append(w + " " + next(it) if w == "-mllvm" else w)
    assert len(set(out)) == len(out), flags
    return set(out)


# (read at import: tests/test_isa_lint_dpp16_resident.py adds entries of its own to isa_lint.FLAGS while it runs)
LISTS = {name: (list(flags), isa_lint.SOURCES.get(name, name)) for name, flags in isa_lint.FLAGS.items()}
LISTS["lqr_dpp16_res"] = (list(res_lint.BASE), "lqr_dpp16")


def test_the_lints_compile_what_the_makefile_compiles():
    assert len(LISTS) >= 14
    for name, (want, source) in sorted(LISTS.items()):
        flags, src = compile_command(name)
        assert flag_set(flags) == flag_set(want), name
        assert src == source + ".hip", name
