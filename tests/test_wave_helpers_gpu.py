"""The wave-wide helpers of the step kernels (csrc/hrgym_device.h: wave_sum, row8_sum, row16_max, wave_max, chain_prefix, subtree_sum, fsqrt, dpp_f64) on the device,
one wave per case through hrg_debug_wave_helpers, against tests/wave_ref.py.  -m gpu.

Every helper equals the reference bit for bit in every active lane, under five EXEC masks (the lanes outside the mask branch around the calls); chain_prefix<true> and
subtree_sum<true>, which trust the caller's zeros instead of masking, over an input that has them.  Exceptions:
  * wave_sum and wave_max return a scalar read from lane 63: that scalar is compared, in every active lane, under the masks that contain lane 63.  Under the other
    two (lanes 0..7, lanes 0..5) v_readlane reads a register lane 63 never wrote -- the helpers leave it undefined, the reference says so, and nothing is compared;
  * the maxima (row16_max, wave_max) are compared by value: of two zeros of opposite sign v_max_f64 may return either, so the sign of a zero result is exempt;
  * dpp_f64_rows (the two row broadcasts under a row mask) leaves the rows outside its row mask undefined: compared in the rows it writes;
  * fsqrt iterates from v_rsq_f64, an approximation with no CPU counterpart: the tap returns that seed, and the reference restates the iteration and the closing
    maximum from it in exact arithmetic rounded once per operation -- bit for bit again, and 0.0 with a positive sign for 0.0, -0.0 and a negative."""
import ctypes

import numpy as np
import pytest

import wave_ref as W
from wave_ref import MASKS, bits as _bits, inputs as _inputs

pytestmark = pytest.mark.gpu


def _fsqrt_input():
    x = np.abs(_inputs()["mixed"]) + 1e-3                       # ordinary lengths
    x[[0, 1, 2, 3, 17, 40, 63]] = [0.0, -0.0, -2.5, 2.5e-300, -0.0, 0.0, -1e-9]   # zeros, negatives, a tiny value far above the denormals
    x[[4, 5, 6]] = [4.0, 1.0, 2.0]
    return x


def _cancel():
    c = np.ones(64)
    c[0], c[16] = 1e16, -1e16
    return c


INPUTS = dict(_inputs(), fsqrt=_fsqrt_input(), cancel=_cancel())


@pytest.fixture(scope="module")
def tap():
    from human_robot_gym_amd._cstruct import CONST
    from human_robot_gym_amd._lib import load_library
    lib = load_library()
    assert CONST["HRG_WAVE_NOUT"] == len(W.ROWS)
    done = {}

    def run(inp, mask):
        if (inp, mask) not in done:
            x = np.ascontiguousarray(INPUTS[inp], np.float64)
            out = np.zeros((len(W.ROWS), 64))
            assert lib.hrg_debug_wave_helpers(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(MASKS[mask]), out.ctypes.data_as(ctypes.c_void_p)) == 0
            done[inp, mask] = dict(zip(W.ROWS, out))
        return done[inp, mask]
    return run


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("inp", INPUTS)
def test_helpers_match_reference(tap, inp, mask):
    x, got = INPUTS[inp], tap(inp, mask)
    act = W.active(MASKS[mask])
    want = W.expected(x, MASKS[mask], seed=got["rsq"])
    assert set(want) | {"rsq"} == set(W.ROWS)
    for name in W.ROWS:
        assert np.isnan(got[name][~act]).all(), name    # an inactive lane wrote nothing
    bad = []
    for name, (vals, check) in want.items():
        if name in W.MAX_ROWS:
            ok = got[name][check] == vals[check]
        else:
            ok = _bits(got[name][check]) == _bits(vals[check])
        if not ok.all():
            lanes = np.flatnonzero(check)[~ok]
            bad.append("%s: lanes %s got %s want %s" % (name, lanes.tolist(), got[name][lanes].tolist(), vals[lanes].tolist()))
    assert not bad, "\n".join(bad)
    # what is compared: everything in every active lane, but the scalars read from lane 63 when that lane is inactive and the rows a broadcast leaves alone
    for name, (vals, check) in want.items():
        if name in ("wave_sum", "wave_max"):
            assert (check == (act if act[63] else np.zeros(64, bool))).all()
        elif name.startswith("dpp_rows_"):
            rows = dict(W.CTRL_ROWS)[int(name[-3:], 16)]
            assert (check == (act & np.array([(rows >> (i >> 4)) & 1 for i in range(64)], bool))).all()
        else:
            assert (check == act).all(), name


def test_fsqrt_is_close_to_the_root(tap):
    """Not the bitwise rule, only a guard that the seed row is v_rsq_f64 (relative error below 2^-23 by the ISA's 2^29 ulp) and that the iteration means a square
    root: the Goldschmidt step squares the seed's error, each correction squares it again, which leaves the rounding of the last operations -- 4 ulp is generous."""
    x, got = INPUTS["fsqrt"], tap("fsqrt", "all")
    pos = x > 0
    assert (np.abs(got["rsq"][pos] * np.sqrt(x[pos]) - 1.0) < 1e-6).all()
    assert (np.abs(got["fsqrt"][pos] - np.sqrt(x[pos])) <= 4 * np.spacing(np.sqrt(x[pos]))).all()
    assert (_bits(got["fsqrt"][~pos]) == _bits(0.0)).all()
