#!/usr/bin/env python3
"""Generate tests/golden/nn_wide_f64.npz: an NNDynamics with more than 16 states (24 states, 6 controls, one hidden
layer of 48 sigmoid units, passthrough, T = 8, B = 5, |u| <= 0.5) through the same recipe as the other nn_* fixtures
(make_golden.nn_case, unchanged: the unmodified reference at random points, along a nominal trajectory, one LQR step
and a whole six-iteration solve).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nn_wide.py

The seed was checked before the fixture was committed (docs/history/r07.md): this package's float32 host-driven solve
on the CPU test backend agrees with `solve_*` well inside the tolerances tests/test_gpu_nn_wide.py applies."""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden  # noqa: E402

SEED = 75

if __name__ == "__main__":
    make_golden.nn_case("nn_wide_f64", SEED, 24, 6, [48], "sigmoid", True, 8, 5, 0.5)
