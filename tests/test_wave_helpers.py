"""tests/wave_ref.py (the lane-by-lane restatement of the kernels' wave helpers that tests/test_wave_helpers_gpu.py holds the device against) against a second,
plain restatement of the same association orders: for a full wave explicit loops over quads, half rows and rows (no lanes, no DPP controls), and under a lane mask
a recursion per lane over the steps, in which an inactive partner counts as 0.0 at EVERY step -- so a masked sum is not the sum over the active lanes: what an
inactive lane would have gathered from its own partners is lost with it.  And for every sum one input where another order gives other bits, so that the device
cannot match the reference by accident."""
import numpy as np
import pytest

import wave_ref as W

from wave_ref import MASKS, bits as _bits, inputs as _inputs


def plain_wave_sum(x):
    quad = [(x[4 * q] + x[4 * q + 1]) + (x[4 * q + 2] + x[4 * q + 3]) for q in range(16)]
    half = [quad[2 * h] + quad[2 * h + 1] for h in range(8)]
    row = [half[2 * r] + half[2 * r + 1] for r in range(4)]
    return (row[3] + row[2]) + (row[1] + row[0])


def plain_row8_sum(x):
    out = np.zeros(64)
    for h in range(8):
        out[8 * h:8 * h + 8] = ((x[8 * h] + x[8 * h + 1]) + (x[8 * h + 2] + x[8 * h + 3])) + ((x[8 * h + 4] + x[8 * h + 5]) + (x[8 * h + 6] + x[8 * h + 7]))
    return out


# ... and lane by lane, by recursion over the steps instead of a pass over the wave per step: what lane i holds after `n` steps is what it held before plus what its
# partner of step n held before, the partner counting as 0.0 when it is inactive or outside the row.  PARTNER: step -> lane -> partner.
BUTTERFLY = (lambda i: i ^ 1, lambda i: i ^ 2, lambda i: i ^ 7, lambda i: i ^ 15)   # the swaps and mirrors as index arithmetic


def shifts(sign):
    return tuple((lambda i, d=d: i + sign * d if (i + sign * d) >> 4 == i >> 4 else -1) for d in (1, 2, 4))


def after(y, act, partner, i, n, op):
    if n == 0:
        return y[i]
    j = partner[n - 1](i)
    return op(after(y, act, partner, i, n - 1, op), after(y, act, partner, j, n - 1, op) if j >= 0 and act[j] else 0.0)


def add(a, b):
    return a + b


def plain_chain_prefix(x, act, i):
    y = [x[k] if k < W.NARM else 0.0 for k in range(64)]
    p = after(y, act, shifts(-1), i, 3, add)
    return p if i < W.NARM else p + x[i]


def plain_subtree_sum(x, act, i):
    y = [x[k] if k < W.NV else 0.0 for k in range(64)]
    return after(y, act, shifts(+1), i, 3, add) if i < W.NARM else x[i]


@pytest.mark.parametrize("inp", ["mixed", "zeros"])
def test_full_wave_orders(inp):
    """With every lane active: quads, then pairs of quads, then the halves of a row, then rows (3 + 2) + (1 + 0)."""
    x = _inputs()[inp]
    assert _bits(W.wave_sum(x)) == _bits(plain_wave_sum(x))
    assert (_bits(W.row8_sum(x)[0]) == _bits(plain_row8_sum(x))).all()
    assert W.wave_max(x) == x.max() and (W.row16_max(x)[0] == np.repeat(x.reshape(4, 16).max(1), 16)).all()


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("inp", ["mixed", "zeros"])
def test_reference_equals_plain_restatement(mask, inp):
    m, x = MASKS[mask], _inputs()[inp].tolist()
    act = W.active(m)
    lanes = [i for i in range(64) if act[i]]
    for ref, plain in ((W.row8_sum, lambda i: after(x, act, BUTTERFLY, i, 3, add)), (W.row16_max, lambda i: after(x, act, BUTTERFLY, i, 4, max)),
                       (W.chain_prefix, lambda i: plain_chain_prefix(x, act, i)), (W.subtree_sum, lambda i: plain_subtree_sum(x, act, i))):
        vals, valid = ref(x, m)
        assert (valid == act).all()
        want = np.array([plain(i) for i in lanes])
        assert (vals[lanes] == want).all() if ref is W.row16_max else (_bits(vals[lanes]) == _bits(want)).all(), ref.__name__
    s, mx = W.wave_sum(x, m), W.wave_max(x, m)
    if not act[63]:
        assert s is None and mx is None   # both are read from lane 63
        return
    for got, op in ((s, add), (mx, max)):
        row = [after(x, act, BUTTERFLY, 16 * r + 15, 4, op) if act[16 * r + 15] else 0.0 for r in range(4)]   # a row's result as its lane 15 broadcasts it
        r3 = op(after(x, act, BUTTERFLY, 63, 4, op), row[2])
        want = op(r3, op(row[1], row[0]) if act[31] else 0.0)
        assert got == want if op is max else _bits(got) == _bits(want)


def test_row_broadcasts_leave_the_other_rows_undefined():
    xv = (np.arange(64.0) + 1, np.ones(64, bool))
    v, ok = W.dpp(xv, W.active(W.FULL), 0x142, 0xA)
    assert ok.reshape(4, 16).all(1).tolist() == [False, True, False, True] and (v[16:32] == 16).all() and (v[48:] == 48).all()
    v, ok = W.dpp(xv, W.active(W.FULL), 0x143, 0xC)
    assert ok.reshape(4, 16).all(1).tolist() == [False, False, True, True] and (v[32:] == 32).all()
    # a disabled source lane supplies 0.0, also to a broadcast
    v, ok = W.dpp(xv, W.active(W.FULL & ~(1 << 47)), 0x142, 0xA)
    assert ok[48:].all() and (v[48:] == 0).all() and (v[16:32] == 16).all()


def test_order_changes_the_bits():
    """One input per sum for which a left-to-right sum, or the same tree with another pairing, has other bits than the helper's order."""
    x = _inputs()["mixed"]
    s = W.wave_sum(x)
    seq = 0.0
    for v in x:
        seq += v
    assert _bits(s) != _bits(seq)
    c = np.ones(64)
    c[0], c[16] = 1e16, -1e16   # the helper's tree rounds ones of rows 0 and 1 away before the two meet; a tree that pairs lanes 0 and 16 first keeps all 62
    assert plain_wave_sum(c.reshape(4, 16).T.ravel()) == 62.0 and W.wave_sum(c) != 62.0
    r8 = W.row8_sum(x)[0]
    assert (_bits(r8[::8]) != _bits([sum(x[8 * h:8 * h + 8].tolist(), 0.0) for h in range(8)])).any()
    cp = W.chain_prefix(x)[0]
    assert (_bits(cp[:W.NARM]) != _bits(np.cumsum(x[:W.NARM]))).any()         # a running sum associates from the left
    st = W.subtree_sum(x)[0]
    right = [sum(x[i:W.NV][::-1].tolist(), 0.0) for i in range(W.NARM)]      # from the leaf inwards
    left = [sum(x[i:W.NV].tolist(), 0.0) for i in range(W.NARM)]
    assert (_bits(st[:W.NARM]) != _bits(right)).any() and (_bits(st[:W.NARM]) != _bits(left)).any()


def test_fsqrt_restatement():
    """From an exact seed the iteration lands on the correctly rounded root; a zero, a negative zero and a negative give +0.0 through the NaN the seed makes of them."""
    for x in (4.0, 2.0, 0.3, 1e-3, 7.25e4, 2.5e-300):
        got = W.fsqrt(x, 1.0 / np.sqrt(x))
        assert abs(got - np.sqrt(x)) <= np.spacing(np.sqrt(x)), x
    for x, seed in ((0.0, np.inf), (-0.0, -np.inf), (-2.0, np.nan)):
        assert _bits(W.fsqrt(x, seed)) == _bits(0.0)
    assert W.fma(2.0 ** 53, 1.0 + 2.0 ** -52, -(2.0 ** 53)) == 2.0                 # the product is not rounded before the sum
    assert W.fma(0.1, 10.0, -1.0) == 2.0 ** -54
