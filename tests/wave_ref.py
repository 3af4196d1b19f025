"""numpy restatement of the wave-wide helpers of csrc/hrgym_device.h (wave_sum, row8_sum, row16_max, wave_max, chain_prefix, subtree_sum, fsqrt, dpp_f64), lane
by lane and step by step in the order of their DPP controls, so that the association order of every sum is the kernel's.  Nothing here is computed by the library.

A wave is 64 lanes = 4 rows of 16.  `mask` is the EXEC mask (bit i = lane i active).  One DPP step moves, into every ACTIVE lane, the value of its source lane; a
source outside the lane's row (row shifts) or an inactive source supplies 0.0.  A lane vector is the pair (values, valid): `valid` is False where the hardware leaves
the value undefined -- an inactive lane, and for the two row broadcasts the rows outside their row mask -- and stays False in whatever is computed from such a lane."""
from fractions import Fraction

import numpy as np

NV, NARM = 8, 6   # HRG_NV, HRG_NARM: degrees of freedom of the robot tree, of which the serial arm
FULL = (1 << 64) - 1
# dpp_f64's controls in the code base (every row), and dpp_f64_rows' (control, row mask)
CTRL_FULL = (0xB1, 0x4E, 0x141, 0x140, 0x111, 0x112, 0x114, 0x101, 0x102, 0x104)
CTRL_ROWS = ((0x142, 0xA), (0x143, 0xC))
# rows of hrg_debug_wave_helpers' output (include/hrgym.h)
ROWS = ("wave_sum", "row8_sum", "row16_max", "wave_max", "chain_prefix", "subtree_sum", "fsqrt") + tuple("dpp_%03X" % c for c in CTRL_FULL) + tuple(
    "dpp_rows_%03X" % c for c, _ in CTRL_ROWS) + ("rsq", "chain_prefix_z", "subtree_sum_z")
MAX_ROWS = ("row16_max", "wave_max")   # compared by value: the sign of a zero is not defined for a maximum of two zeros


def active(mask):
    return np.array([(mask >> i) & 1 for i in range(64)], bool)


def source(ctrl, i):
    """The lane that lane i reads under DPP control `ctrl`; -1: outside the row (a zero is shifted in) or no source (row 0 of row_bcast15, rows 0, 1 of row_bcast31)."""
    row, k = i & ~15, i & 15
    if ctrl <= 0xFF:                                   # quad_perm: two bits per lane of the quad
        return (i & ~3) | ((ctrl >> (2 * (i & 3))) & 3)
    if 0x101 <= ctrl <= 0x10F:                         # row_shl:n -- lane i reads lane i + n
        return row + k + (ctrl & 15) if k + (ctrl & 15) < 16 else -1
    if 0x111 <= ctrl <= 0x11F:                         # row_shr:n -- lane i reads lane i - n
        return row + k - (ctrl & 15) if k - (ctrl & 15) >= 0 else -1
    if ctrl == 0x140:                                  # row_mirror
        return row + 15 - k
    if ctrl == 0x141:                                  # row_half_mirror
        return (i & ~7) + 7 - (i & 7)
    if ctrl == 0x142:                                  # row_bcast15: lane 15 of a row to the next row
        return row - 1 if row else -1
    if ctrl == 0x143:                                  # row_bcast31: lane 31 to rows 2 and 3
        return 31 if i >= 32 else -1
    raise ValueError(hex(ctrl))


def dpp(v, act, ctrl, row_mask=0xF):
    vals, valid = v
    out, ok = np.zeros(64), np.zeros(64, bool)
    for i in range(64):
        if not act[i] or not (row_mask >> (i >> 4)) & 1:
            out[i] = np.nan
            continue
        s = source(ctrl, i)
        if s < 0 or not act[s]:
            out[i], ok[i] = 0.0, True
        else:
            out[i], ok[i] = vals[s], valid[s]
    return out, ok


def _lanes(x, act):
    return np.where(act, np.asarray(x, np.float64), np.nan), act.copy()


def _add(a, b):
    with np.errstate(invalid="ignore"):
        return a[0] + b[0], a[1] & b[1]


def _max(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(a[0] > b[0], a[0], b[0]), a[1] & b[1]


def _where(cond, a, b):
    return np.where(cond, a[0], b[0]), np.where(cond, a[1], b[1])


def _last_lane(v):
    """The scalar wave_sum / wave_max return: lane 63's value; None where that is undefined (lane 63 inactive: v_readlane reads a register the lane never wrote)."""
    return float(v[0][63]) if v[1][63] else None


def wave_sum(x, mask=FULL):
    act = active(mask)
    v = _lanes(x, act)
    for ctrl in (0xB1, 0x4E, 0x141, 0x140):
        v = _add(v, dpp(v, act, ctrl))
    for ctrl, rows in CTRL_ROWS:
        v = _add(v, dpp(v, act, ctrl, rows))
    return _last_lane(v)


def row8_sum(x, mask=FULL):
    act = active(mask)
    v = _lanes(x, act)
    for ctrl in (0xB1, 0x4E, 0x141):
        v = _add(v, dpp(v, act, ctrl))
    return v


def row16_max(x, mask=FULL):
    act = active(mask)
    v = _lanes(x, act)
    for ctrl in (0xB1, 0x4E, 0x141, 0x140):
        v = _max(dpp(v, act, ctrl), v)
    return v


def wave_max(x, mask=FULL):
    act = active(mask)
    v = row16_max(x, mask)
    for ctrl, rows in CTRL_ROWS:
        v = _max(dpp(v, act, ctrl, rows), v)
    return _last_lane(v)


def chain_prefix(x, mask=FULL):
    act, lane = active(mask), np.arange(64)
    xv = _lanes(x, act)
    y = _where(lane < NARM, xv, (np.zeros(64), act.copy()))
    for ctrl in (0x111, 0x112, 0x114):
        y = _add(y, dpp(y, act, ctrl))
    return _where(lane < NARM, y, _add(y, xv))


def subtree_sum(x, mask=FULL):
    act, lane = active(mask), np.arange(64)
    xv = _lanes(x, act)
    y = _where(lane < NV, xv, (np.zeros(64), act.copy()))
    for ctrl in (0x101, 0x102, 0x104):
        y = _add(y, dpp(y, act, ctrl))
    return _where(lane < NARM, y, xv)


def fma(a, b, c):
    """a * b + c rounded once (v_fma_f64)."""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fsqrt(x, seed):
    """fsqrt's iteration restated from the value of v_rsq_f64(x) (`seed`, a hardware approximation that has no CPU counterpart): one Goldschmidt step, two residual
    corrections, and 0.0 for every x that is not positive -- the seed of a zero or a negative makes g a NaN, which the closing maximum with 0.0 drops."""
    x, y = float(x), float(seed)
    with np.errstate(invalid="ignore", over="ignore"):
        g, h = float(np.float64(x) * np.float64(y)), float(np.float64(0.5) * np.float64(y))
    r = fma(-h, g, 0.5)
    g, h = fma(g, r, g), fma(h, r, h)
    g = fma(fma(-g, g, x), h, g)
    g = fma(fma(-g, g, x), h, g)
    return 0.0 if np.isnan(g) or g <= 0.0 else g


def expected(x, mask, seed=None):
    """{row of hrg_debug_wave_helpers: (values[64], check[64])}: what every lane must hold, and the lanes where that is defined.  `seed`: the rsq row of the
    output under test (for the fsqrt row; left out without it)."""
    act = active(mask)
    out = {}
    for name, s in (("wave_sum", wave_sum(x, mask)), ("wave_max", wave_max(x, mask))):
        out[name] = (np.full(64, np.nan if s is None else s), act if s is not None else np.zeros(64, bool))
    out["row8_sum"], out["row16_max"] = row8_sum(x, mask), row16_max(x, mask)
    out["chain_prefix"], out["subtree_sum"] = chain_prefix(x, mask), subtree_sum(x, mask)
    lane = np.arange(64)   # chain_prefix<true> / subtree_sum<true>: the same sums over an input that is 0.0 where the plain forms would mask it
    out["chain_prefix_z"] = chain_prefix(np.where(lane < NARM, x, 0.0), mask)
    out["subtree_sum_z"] = subtree_sum(np.where(lane < NV, x, 0.0), mask)
    xv = _lanes(x, act)
    for c in CTRL_FULL:
        out["dpp_%03X" % c] = dpp(xv, act, c)
    for c, rows in CTRL_ROWS:
        out["dpp_rows_%03X" % c] = dpp(xv, act, c, rows)
    if seed is not None:
        out["fsqrt"] = (np.array([fsqrt(x[i], seed[i]) if act[i] else np.nan for i in range(64)]), act.copy())
    return out


# ---- the cases the CPU and the GPU test share: EXEC masks (all lanes | lanes 0..7 | lanes 0..5 | row 2 and the upper half of row 3 | holes inside rows, lanes 15 and
#      47 -- sources of row_bcast15 -- among them) and inputs (mixed sign and magnitude, so that the order of a sum shows in its bits | exact zeros of both signs)
MASKS = {"all": FULL, "lanes0-7": 0xFF, "lanes0-5": 0x3F, "row2+half3": (0xFFFF << 32) | (0xFF << 56),
         "holes": FULL & ~sum(1 << i for i in (3, 9, 10, 15, 22, 36, 47, 50, 61))}


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def inputs():
    rng = np.random.RandomState(11)
    x = rng.normal(size=64) * 10.0 ** rng.uniform(-3, 3, 64)
    z = np.where(np.arange(64) % 3 == 0, 0.0, np.where(np.arange(64) % 3 == 1, -0.0, rng.normal(size=64)))
    return {"mixed": x, "zeros": z}
