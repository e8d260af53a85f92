"""The inputs of tests/test_gpu_flip_windows.py built without a GPU: tests/_flip_window_cases.py asserts its conditions on the inputs (margins of
the uniforms, flips in both directions, panels beyond 128 rows) from the longdouble reference alone while it builds a case.  Three of the
eleven cases are built here -- a compiled block size, the run-time one with an odd window boundary, the one whose window the LDS cap cuts --
the GPU module builds all of them, with the same assertions, before it launches anything."""
import numpy as np
import pytest

from tests import _dense_ref as R
from tests import _flip_window_cases as C


def test_window_lengths_come_from_the_library():
    assert [C.window_blocks(B) for B in C.BLOCK_SIZES] == [320, 160, 106, 80, 64, 53, 45, 40, 29, 20, 5]
    assert (C.window_blocks(11) * 11) % 2 == 1 and (C.window_blocks(7) * 7) % 2 == 1 and (C.window_blocks(16) * 16) % 2 == 0


@pytest.mark.parametrize("B", [8, 11, 32])
def test_case_meets_its_input_conditions(B):
    case = C.build_case(B)                      # (asserts the conditions)
    Rw, N = case["R"], case["N"]
    assert N == 2 * Rw + 3 and case["nwin"] == 3 and abs(int(case["a0"].sum()) - N / 2) <= 1
    every = case["neurons"]["everything"]["ref"]
    assert [len(f) for f in every["win_flips"]] == [Rw, Rw, 3]                       # (at these seeds every block flips)
    mixed = case["neurons"]["mixed"]["ref"]
    # the snapshots are the serial chain's: the last one is the sweep of the initial tableau on the net set of flipped blocks
    net = sorted(m for m in range(N) if mixed["a"][m] != case["a0"][m])
    rows = [m * B + b for m in net for b in range(B)]
    sg = np.repeat([1.0 if mixed["a"][m] else -1.0 for m in net], B)
    direct = R.sweep_block(R.ld(case["M0"]), rows, sg)
    assert R.relerr(np.asarray(mixed["snaps"][-1][0], dtype=np.float64), direct) < 1e-13
    assert all(k > 0 for k in mixed["kappa"][:2]) and max(mixed["kappa"] + every["kappa"]) < 10
