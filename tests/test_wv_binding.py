"""CPU-only, compiles nothing: the gfx950 binding of the `wv::` lane interface has ONE definition per name.

The fused kernel bodies (csrc/lqr_*_body.h, lqr_small_math.h) are written against `wv::`; csrc/wv_gfx950.h binds the names whose gfx950 form
is shared, and lqr_dpp16.hip, lqr_mfma40.hip, lqr_mfma16.hip and lqr_wave1_wv.h add what only their kernel uses.  This test reads every
`namespace wv { ... }` under csrc/ (not the emulator's, tests/emu/) and holds that
  * a function name is defined in exactly one file -- overloads and specialisations of a name stay together --
  * unless it stands in PER_KERNEL below, next to the reason why kernels bind it differently;
  * every PER_KERNEL name really is defined in two files or more (the list cannot rot);
  * every PER_KERNEL name stands in the second list of wv_gfx950.h's opening comment, "the names a kernel binds for itself".
docs/history/r30.md has what this printed on the tree before the shared header (35 names in more than one file, 28 of them outside PER_KERNEL)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc.pytorch_amd", "csrc")
SHARED = "wv_gfx950.h"

# name -> why it has more than one gfx950 definition (the header's second list says what each kernel's form is)
PER_KERNEL = {
    "rcp": "raw v_rcp_f32 in the 12/4 kernel (instruction-count bound), v_rcp_f32 + a Newton step in the 32/8 and one-problem-per-wavefront kernels",
    "uniform": "v_readfirstlane where a wavefront is one problem; the identity in the 12/4 kernel, where a row is a problem",
    "readlane": "v_readlane as it comes, behind a v_readfirstlane of the index (12/4), or __shfl with a per-lane index (row-per-problem)",
    "readlane_f64": "the two halves through readfirstlane + v_readlane (12/4) or through __shfl (row-per-problem)",
    "lds_sync": "a compiler barrier where DS order suffices; fence + wave barrier in the row-per-problem kernel, whose LDS is a plain float array",
    "fmac_bcast": "s_nop + v_fmac_f32_dpp in asm; compiler-visible fmaf(bcast) in the row-per-problem kernel (measured 4 % faster there)",
    "row_sum_f64": "DPP steps on the halves in row_sum's order (12/4); __shfl_xor steps in another order of additions (row-per-problem)",
}

DEFINITION = re.compile(r"\bMPC_DEV\s+[^(;{}]*?(\w+)\s*(?:<[^<>()]*>)?\s*\(")


def code(path):
    """The file's text with // comments cut off (line structure kept)."""
    return "\n".join(l.split("//")[0] for l in open(path, errors="replace").read().split("\n"))


def closing(text, at, pair):
    """Index of the bracket that closes the one at text[at]."""
    depth = 0
    for i in range(at, len(text)):
        depth += (text[i] == pair[0]) - (text[i] == pair[1])
        if depth == 0:
            return i
    raise AssertionError("unbalanced %s" % pair)


def wv_definitions(path):
    """The names of the functions DEFINED (a body, not a declaration) in the file's `namespace wv` blocks, one entry per definition."""
    text, out = code(path), []
    for ns in re.finditer(r"\bnamespace\s+wv\s*\{", text):
        block = text[ns.end() - 1:closing(text, ns.end() - 1, "{}") + 1]
        for m in DEFINITION.finditer(block):
            after = block[closing(block, m.end() - 1, "()") + 1:].lstrip()
            if after.startswith("{"):
                out.append(m.group(1))
    return out


def bindings():
    """{file name: [defined names]} of the files under csrc/ that have a namespace wv."""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        names = wv_definitions(path)
        if names:
            out[os.path.basename(path)] = names
    return out


def files_of():
    where = {}
    for f, names in bindings().items():
        for n in set(names):
            where.setdefault(n, []).append(f)
    return where


def test_one_definition_per_name():
    b = bindings()
    print({f: len(n) for f, n in b.items()})
    twice = {n: fs for n, fs in files_of().items() if len(fs) > 1 and n not in PER_KERNEL}
    assert not twice, "%d wv:: names are defined in more than one file and are not in PER_KERNEL: %s" % (
        len(twice), "; ".join("%s (%s)" % (n, ", ".join(fs)) for n, fs in sorted(twice.items())))
    # (the parser still finds the bindings, the shared part among them)
    assert set(b) == {SHARED, "lqr_dpp16.hip", "lqr_mfma40.hip", "lqr_mfma16.hip", "lqr_wave1_wv.h"}, sorted(b)
    assert len(set(b[SHARED])) >= 25, b[SHARED]


def test_per_kernel_names_are_bound_per_kernel():
    where = files_of()
    for name in sorted(PER_KERNEL):
        assert len(where.get(name, [])) >= 2, "%s is defined in %s: drop it from PER_KERNEL" % (name, where.get(name, "no file"))


def test_per_kernel_names_are_in_the_headers_list():
    text = open(os.path.join(CSRC, SHARED)).read()
    head = text[:text.index("#pragma once")]
    second = head[head.index("the names a kernel binds for itself"):]
    for name in sorted(PER_KERNEL):
        assert re.search(r"^//   [\w(), <>]*\b%s\b" % name, second, re.M), "%s has no entry in the second list of %s" % (name, SHARED)
