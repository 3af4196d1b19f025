"""cull_box (csrc/hrgym_device.h), the box around the robot's capsules that collide and shield_step cull the human's capsules against, on the device: one wave per case
through hrg_debug_cull_box, against numpy's min and max (tests/cull_box_ref.py).  -m gpu.

The six bounds must equal numpy's exactly, for n = 1, 7, 10, 16 capsules: random ones, degenerate ones (p1 = p2), coordinates of +0.0 and -0.0, extents of 1e-300 and
1e+300.  Only the sign of a bound that is zero is free (of two zeros of opposite sign v_max_f64 may return either), so the comparison is by value.  The rows of the
input behind the first n are NaN: a kernel that read one would return it."""
import ctypes

import numpy as np
import pytest

import cull_box_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()


@pytest.fixture(scope="module")
def tap():
    import torch  # noqa: F401  (first: the library must bind to the HIP runtime torch ships, also when a test with a HipBatch follows in this process)
    from human_robot_gym_amd._lib import load_library
    lib = load_library()

    def run(caps, n):
        x = np.array(caps, np.float64, order="C")
        assert x.shape == (16, 7)
        x[n:] = np.nan
        out = np.full(6, np.nan)
        assert lib.hrg_debug_cull_box(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int32(n), out.ctypes.data_as(ctypes.c_void_p)) == 0
        return out[:3], out[3:]
    return run


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_box_equals_numpy(tap, case, n):
    lo, hi = tap(CASES[case], n)
    wlo, whi = R.box_numpy(CASES[case], n)
    print(case, n, "lo", lo.tolist(), "hi", hi.tolist())
    assert (lo == wlo).all() and (hi == whi).all(), f"{case} n={n}: lo {lo.tolist()} want {wlo.tolist()}; hi {hi.tolist()} want {whi.tolist()}"


def test_n_outside_one_row_is_refused(tap):
    from human_robot_gym_amd._lib import load_library
    lib = load_library()
    x, out = np.zeros((16, 7)), np.zeros(6)
    for n in (0, 17, -1):
        assert lib.hrg_debug_cull_box(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int32(n), out.ctypes.data_as(ctypes.c_void_p)) != 0
