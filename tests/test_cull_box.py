"""tests/cull_box_ref.py on its own (no GPU): the lane layout of cull_box (c = l & 15, g = l >> 4) serves every capsule and every one of the six bounds exactly once, a
lane without a capsule holds the empty value, and the bounds that come out of the layout are numpy's min and max over the capsules."""
import numpy as np
import pytest

import cull_box_ref as R


@pytest.mark.parametrize("n", R.NS)
def test_layout_covers_every_capsule_and_bound_once(n):
    seen = {}
    for lane in range(64):
        c, r1, r2 = R.lane_role(lane, n)
        assert (c is None) == ((lane & 15) >= n)
        if c is None:
            continue
        for role in (r1, r2):
            if role is not None:
                seen[c, role] = seen.get((c, role), 0) + 1
    want = {(c, (axis, neg)) for c in range(n) for axis in range(3) for neg in (False, True)}
    assert set(seen) == want and set(seen.values()) == {1}
    # the rows of the reductions: quantity g of the first pass sits in row g, the z bounds in rows 0 and 1 of the second
    assert [R.PASS1[g] for g in range(4)] == [(0, False), (0, True), (1, False), (1, True)] and R.PASS2 == ((2, False), (2, True), None, None)


@pytest.mark.parametrize("n", R.NS)
def test_lanes_without_a_capsule_hold_the_empty_value(n):
    e1, e2 = R.lane_values(R.cases()["random"], n)
    for lane in range(64):
        has = (lane & 15) < n
        assert (e1[lane] != R.EMPTY) == has
        assert (e2[lane] != R.EMPTY) == (has and lane < 32)


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("case", sorted(R.cases()))
def test_layout_gives_numpy_min_and_max(case, n):
    caps = R.cases()[case]
    lo, hi = R.box_by_lanes(caps, n)
    wlo, whi = R.box_numpy(caps, n)
    assert (lo == wlo).all() and (hi == whi).all(), (lo, wlo, hi, whi)   # by value: the sign of a zero bound is free
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
