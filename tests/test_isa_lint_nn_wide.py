"""Static checks on the gfx950 assembly of the two-state-tile network kernels (csrc/nn_dynamics.hip, 16 < n_state <= 32;
no GPU: hipcc cross-compiles).  The second state tile lives in registers next to the first -- so the instantiations
must still fit the register file without scratch memory, and every layer product must still be on the matrix core."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import test_isa_lint  # noqa: E402

pytestmark = test_isa_lint.pytestmark           # the same condition as the existing lint: needs hipcc

WIDE = ("nn_wide_rollout_kernel", "nn_wide_linearize_kernel")


def _bodies():
    """{kernel symbol: its lines of assembly} for the wide kernels, and the whole text"""
    import isa_lint
    lines = isa_lint.assembly("nn_dynamics")
    kernels, _ = isa_lint.structure(lines)
    out = {}
    for idx, (start, name) in enumerate(kernels):
        if any(w in name for w in WIDE):
            end = kernels[idx + 1][0] if idx + 1 < len(kernels) else len(lines)
            # (a kernel's code ends at its .Lfunc_end label; the next symbol may be far behind the metadata)
            for j in range(start, end):
                if lines[j].startswith(".Lfunc_end"):
                    end = j
                    break
            out[name] = lines[start:end]
    return out, "\n".join(lines)


def test_wide_network_kernels_exist_once_per_weight_placement():
    """nn_wide_rollout_kernel<WL> and nn_wide_linearize_kernel<WL>, WL = weights in LDS / in global memory: two each."""
    bodies, _ = _bodies()
    for w in WIDE:
        names = sorted(n for n in bodies if w in n)
        assert len(names) == 2, (w, names)
        assert any("ILb1E" in n for n in names) and any("ILb0E" in n for n in names), names


def test_wide_network_kernels_stay_in_registers():
    """No scratch instruction in the wide kernels, no spilled vector register in their code object notes."""
    bodies, text = _bodies()
    assert len(bodies) == 4
    for name, body in bodies.items():
        assert not any("scratch_" in l and not l.strip().startswith(";") for l in body), name
    seen = 0
    for block in text.split("- .agpr_count")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", block)
        if nm and nm.group(1) in bodies:
            seen += 1
            assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, nm.group(1)
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, nm.group(1)
    assert seen == 4


def test_wide_network_kernels_run_their_layers_on_the_matrix_core():
    bodies, _ = _bodies()
    assert len(bodies) == 4
    for name, body in bodies.items():
        # (at least the four accumulation chains of one layer loop)
        n = sum(l.strip().startswith("v_mfma_f32_16x16x4") for l in body)
        assert n >= 4, (name, n)
