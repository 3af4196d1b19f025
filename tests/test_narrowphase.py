"""The primitive narrowphase of the oracle (seg_seg, seg_box, cap_box_two, box_box2 through their hrgo_test_* taps) against the exact geometric reference and the
checker of tests/narrowphase_ref.py, on the cases of tests/narrowphase_cases.py.  The device runs the same cases through the same checker in
tests/test_narrowphase_gpu.py.

Where the 1e-12 m comes from: the coordinates are metre-sized doubles (2.2e-16 relative, a few dozen operations deep: 1e-14), and seg_box stops its Newton iteration
once the slope has fallen below 1e-13 of its range, which leaves at most 1e-13 L at a touching pair.  Measured: DESIGN.md section 2d."""
import numpy as np
import pytest

import narrowphase_cases as nc
import narrowphase_ref as nr
from narrowphase_ref import BOXBOX, CAPBOX, CHECK, F64, LD, SEGBOX, SEGSEG

H = nc.CUBE[0]
KIND_NAMES = {v: k for k, v in nr.KINDS.items()}


# ------------------------------------------------------------------------------------------------ anchors of the reference itself
def test_reference_hand_values():
    # segments: crossing, parallel, an end against an interior, skew lines with a known common perpendicular
    assert nr.seg_seg_ref([-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0])["d"] == 0
    assert nr.seg_seg_ref([0, 0, 0], [1, 0, 0], [0.2, 0.3, 0], [0.7, 0.3, 0])["d"] == 0.3
    np.testing.assert_allclose(nr.seg_seg_ref([0, 0, 0], [1, 0, 0], [2, 1, 0], [3, 5, 0])["d"], np.sqrt(2), rtol=1e-15)
    np.testing.assert_allclose(nr.seg_seg_ref([-1, 0, 0], [1, 0, 0], [0, -1, 0.25], [0, 1, 0.25])["d"], 0.25, rtol=1e-15)
    assert nr.seg_seg_ref([1, 2, 3], [1, 2, 3], [1, 2, 7], [1, 2, 7])["d"] == 4
    # segment - box: over a face, beyond an edge, beyond a corner, through the box; a yawed box
    h = [0.1, 0.2, 0.3]
    assert nr.seg_box_ref([-0.05, 0, 0.5], [0.05, 0.1, 0.5], [0, 0, 0], nc.ID, h)["d"] == 0.2
    np.testing.assert_allclose(nr.seg_box_ref([-1, 0.5, 0.7], [1, 0.5, 0.7], [0, 0, 0], nc.ID, h)["d"], np.hypot(0.3, 0.4), rtol=1e-15)
    np.testing.assert_allclose(nr.seg_box_ref([0.2, 0.3, 0.4], [0.5, 0.9, 0.8], [0, 0, 0], nc.ID, h)["d"], 0.1 * np.sqrt(3), rtol=1e-15)
    assert nr.seg_box_ref([-1, 0, 0], [1, 0.1, 0.1], [0, 0, 0], nc.ID, h)["d"] == 0
    # a segment that dips towards an edge between its ends: the stationary point inside a piece
    np.testing.assert_allclose(nr.seg_box_ref([0.3, -1, 0.3], [0.3, 1, 0.3], [0, 0, 0], nc.ID, [0.1, 0.1, 0.1])["d"], 0.2 * np.sqrt(2), rtol=1e-15)
    np.testing.assert_allclose(nr.seg_box_ref([1, -1, 0], [1, 1, 0], [0, 0, 0], nc.quat([0, 0, 1], np.pi / 4), [0.5, 0.5, 0.5])["d"], 1 - 0.5 * np.sqrt(2), rtol=1e-14)
    # the stretch of a capsule lying over a face and overhanging one edge: from its own end to the edge
    s = nr.cap_box_ref([-0.05, 0, 0.32], [0.15, 0, 0.32], [0, 0, 0], nc.ID, h, 0.03)
    assert s["two"] and s["sure"] and s["kn"] == 2 and s["lo"] == 0 and abs(s["hi"] - 0.75) <= s["step"]
    assert not nr.cap_box_ref([-0.05, 0, 0.34], [0.15, 0, 0.34], [0, 0, 0], nc.ID, h, 0.03)["two"]          # farther than r
    # boxes: aligned cubes overlap by the penetration on z and by an edge on x and y; the 45 degree octagon; the parallelogram of the finding
    ax = nr.sat_axes([0, 0, 0], nc.ID, nc.CUBE, [0, 0, 2 * H - 4e-4], nc.ID, nc.CUBE)
    np.testing.assert_allclose([a["s"] for a in ax[:6]], [-2 * H, -2 * H, -4e-4] * 2, rtol=1e-12)
    assert all(a["n"][2] == 1 for a in (ax[2], ax[5])) and len(ax) == 12         # oriented from a to b; the three pairs of parallel edges give no axis
    box = lambda p, q, h_: (np.asarray(p, float), np.asarray(q, float), np.asarray(h_, float))  # noqa: E731
    P, area = nr.overlap_polygon(box([0, 0, 0], nc.ID, nc.CUBE), box([0, 0, 2 * H], nc.quat([0, 0, 1], np.pi / 4), nc.CUBE), 2, np.array([0, 0, 1.0]))
    assert len(P) == 8
    np.testing.assert_allclose(area, 8 * (np.sqrt(2) - 1) * H * H, rtol=1e-14)
    f = nc.FINDING
    P, area = nr.overlap_polygon(box([0, 0, 0], nc.ID, f["ha"]), box([f["xy"][0], f["xy"][1], f["ha"][2] + f["hb"][2]], nc.quat([0, 0, 1], f["yaw"]), f["hb"]), 2, np.array([0, 0, 1.0]))
    S, knife = nr.significant_vertices(P, 1e-6 * np.hypot(*f["ha"][:2]))
    assert len(P) == 4 and len(S) == 4 and not knife
    np.testing.assert_allclose(P[1] - P[0], P[2] - P[3], atol=1e-15)               # a parallelogram
    np.testing.assert_allclose(nr.box_corners([1, 2, 3], nc.ID, [1, 1, 1]).mean(0), [1, 2, 3])


@pytest.mark.parametrize("kind", [SEGSEG, SEGBOX, CAPBOX, BOXBOX])
def test_reference_float64_against_long_double(kind):
    """the float64 path of the reference against its long double path: its own error, which the 1e-12 of the checker has to dwarf"""
    names, Q = nc.CASES[kind]()
    worst = 0.0
    for q in Q[::7]:
        if kind == SEGSEG:
            a, b = (nr.seg_seg_ref(**nr.unpack(kind, q, dt), dt=dt)["d"] for dt in (F64, LD))
        elif kind in (SEGBOX, CAPBOX):
            u = nr.unpack(kind, q)
            a, b = (nr.seg_box_ref(u["p1"], u["p2"], u["c"], u["quat"], u["hb"], dt)["d"] for dt in (F64, LD))
        else:   # (an edge pair's axis is a normalised cross product: conditioned as 1 / |A_i x B_j|, so the well-conditioned ones are compared here)
            a, b = (np.array([x["s"] for x in nr.sat_axes(**nr.unpack(kind, q, dt), dt=dt) if x["l2"] > 1e-4]) for dt in (F64, LD))
        worst = max(worst, float(np.max(np.abs(np.asarray(a, LD) - b))))
    print(f"[narrowphase] reference {KIND_NAMES[kind]}: float64 against long double differ by at most {worst:.3g} m")
    assert worst <= 1e-14


def test_reference_symmetries():
    """swapping the two bodies and moving both by one rigid motion leave distances, overlaps and areas where they are"""
    c, qm = nc.GENERIC
    R = nr.quat_mat(qm)
    mv = lambda x: c + R @ x  # noqa: E731
    _, Q = nc.seg_seg_cases()
    for q in Q[::23]:
        u = nr.unpack(SEGSEG, q)
        d = nr.seg_seg_ref(**u)["d"]
        assert abs(nr.seg_seg_ref(u["p2"], u["q2"], u["p1"], u["q1"])["d"] - d) <= 1e-15
        assert abs(nr.seg_seg_ref(*(mv(u[k]) for k in ("p1", "q1", "p2", "q2")))["d"] - d) <= 1e-14
    _, Q = nc.seg_box_cases()
    for q in Q[::23]:
        u = nr.unpack(SEGBOX, q)
        d = nr.seg_box_ref(u["p1"], u["p2"], u["c"], u["quat"], u["hb"])["d"]
        assert abs(nr.seg_box_ref(u["p2"], u["p1"], u["c"], u["quat"], u["hb"])["d"] - d) <= 1e-15
        assert abs(nr.seg_box_ref(mv(u["p1"]), mv(u["p2"]), mv(u["c"]), nc.qmul(qm, u["quat"]), u["hb"])["d"] - d) <= 1e-14
    _, Q = nc.box_box_cases()
    for q in Q[::23]:
        u = nr.unpack(BOXBOX, q)
        s = sorted(float(a["s"]) for a in nr.sat_axes(**u) if a["l2"] > 1e-4)
        sw = sorted(float(a["s"]) for a in nr.sat_axes(u["pb"], u["qb"], u["hb"], u["pa"], u["qa"], u["ha"]) if a["l2"] > 1e-4)
        mo = sorted(float(a["s"]) for a in nr.sat_axes(mv(u["pa"]), nc.qmul(qm, u["qa"]), u["ha"], mv(u["pb"]), nc.qmul(qm, u["qb"]), u["hb"]) if a["l2"] > 1e-4)
        np.testing.assert_allclose(sw, s, atol=1e-14)
        np.testing.assert_allclose(mo, s, atol=1e-14)


# ------------------------------------------------------------------------------------------------ the generator, the oracle
def judge(kind, Q, out, names, who):
    """every output through the checker: asserts that none is flagged and that at most 1 % of the cases sat on a knife edge; returns the verdicts"""
    V = [CHECK[kind](q, o) for q, o in zip(Q, out)]
    bad = [f"{name}: {v.bad[0]}" for name, v in zip(names, V) if v.bad]
    knife = float(np.mean([v.knife or (kind == BOXBOX and v.free) for v in V]))   # (a box pair whose contact order is free leaves the side-by-side comparison of the order)
    err = max((abs(v.stats["err"]) for v in V if "err" in v.stats and not v.stats.get("banded")), default=0.0)
    ratios = [v.stats["ratio"] for v in V if "ratio" in v.stats and v.stats.get("corners", 0) >= 3]
    print(f"[narrowphase] {who} {KIND_NAMES[kind]}: {len(Q)} cases, {len(bad)} flagged, knife edges {knife:.4f}, largest error {err:.3g} m"
          + (f", smallest kept share of an overlap polygon {min(ratios):.4f}" if ratios else ""))
    assert not bad, f"{who} {KIND_NAMES[kind]}: {len(bad)} of {len(Q)} outputs flagged, first: {bad[:5]}"
    assert knife <= 0.01, f"{KIND_NAMES[kind]}: {knife:.3f} of the cases sit on a knife edge (at most 1 % may be left out of the exact comparison)"
    return V


@pytest.mark.parametrize("kind", [SEGSEG, SEGBOX, CAPBOX, BOXBOX])
def test_oracle_against_the_reference(oracle_lib, kind):
    names, Q = nc.CASES[kind]()
    assert len(Q) <= 2000 and len(set(names)) == len(names)
    V = judge(kind, Q, nc.oracle_outputs(oracle_lib, kind, Q), names, "oracle")
    if kind == CAPBOX:   # both answers are exercised, and most cases decide with the 2 % margin
        two = np.array([v.stats["two"] for v in V])
        assert 0.2 < two.mean() < 0.8
    if kind == BOXBOX:   # every count, face and edge contacts
        assert {v.stats["n"] for v in V} == {0, 1, 2, 3, 4}


def test_the_finding_keeps_its_four_corners(oracle_lib):
    """a board lying across an edge at a yaw: the overlap is a parallelogram whose longest distance from the first kept corner is to an adjacent one"""
    names, Q = nc.box_box_cases()
    for k in (k for k, name in enumerate(names) if name.startswith("the parallelogram of the finding")):
        out = nc.oracle_outputs(oracle_lib, BOXBOX, Q[k:k + 1])[0]
        V = nr.check_box_box(Q[k], out)
        assert out[0] == 4 and not V.bad and V.stats["corners"] == 4 and V.stats["ratio"] > 1 - 1e-9, (names[k], V.bad, V.stats)


# ------------------------------------------------------------------------------------------------ teeth: the checker flags what is wrong
def _case(kind, name):
    names, Q = nc.CASES[kind]()
    return Q[names.index(name)]


def _flagged(kind, q, out, **kw):
    return bool(CHECK[kind](q, out, **kw).bad)


def test_teeth(oracle_lib):
    run = lambda kind, q: nc.oracle_outputs(oracle_lib, kind, q[None])[0]  # noqa: E731
    # a correct output with a witness moved by 1e-9
    q = _case(SEGSEG, "crossing, skew/posed")
    out = run(SEGSEG, q)
    assert not _flagged(SEGSEG, q, out)
    d1, d2 = q[3:6] - q[0:3], q[9:12] - q[6:9]
    off = np.cross(d1, d2) / np.linalg.norm(np.cross(d1, d2))
    for sl in (slice(1, 4), slice(4, 7)):
        o = out.copy()
        o[sl] += 1e-9 * off
        assert _flagged(SEGSEG, q, o)
    q = _case(SEGBOX, f"closest inside, over a face h={nc.HEAD}/posed")
    out = run(SEGBOX, q)
    assert not _flagged(SEGBOX, q, out)
    nrm = (out[1:4] - out[4:7]) / np.linalg.norm(out[1:4] - out[4:7])
    for sl in (slice(1, 4), slice(4, 7)):
        o = out.copy()
        o[sl] += 1e-9 * nrm
        assert _flagged(SEGBOX, q, o)
    o = out.copy()
    o[0] = (np.sqrt(out[0]) + 1e-9) ** 2          # ... or the distance itself
    assert _flagged(SEGBOX, q, o)
    q = _case(BOXBOX, "the parallelogram of the finding, posed")
    out = run(BOXBOX, q)
    assert out[0] == 4 and not _flagged(BOXBOX, q, out)
    o = out.copy()
    o[1:4] += 1e-9 * out[4:7]
    assert _flagged(BOXBOX, q, o)
    # a flipped normal
    o = out.copy()
    o[1:29].reshape(4, 7)[:, 3:6] *= -1
    assert _flagged(BOXBOX, q, o)
    # one contact dropped: what the rule kept before the fourth contact was added (three corners, half the parallelogram)
    for drop in range(4):
        o = out.copy()
        c = np.delete(out[1:29].reshape(4, 7), drop, axis=0)
        o[0], o[1:29] = 3, np.concatenate([c.ravel(), np.zeros(7)])
        V = nr.check_box_box(q, o)
        assert V.bad and abs(V.stats["ratio"] - 0.5) < 1e-9
        assert not nr.check_box_box(q, o, fixed=False).bad     # (a quarter of the polygon is all the earlier rule promises)
    # a contact moved outside the polygon
    R = nr.quat_mat(q[3:7])
    for shift in (1e-3, 1e-9):
        o = out.copy()
        o[1:4] += shift * R[:, 0]
        assert _flagged(BOXBOX, q, o)
    # a depth scaled by 1.1
    o = out.copy()
    o[1:29].reshape(4, 7)[:, 6] *= 1.1
    assert _flagged(BOXBOX, q, o)
    q = _case(BOXBOX, "cube on cube: crossed edges at 60 deg, 0.0005")
    out = run(BOXBOX, q)
    assert out[0] == 1 and not _flagged(BOXBOX, q, out)
    o = out.copy()
    o[7] *= 1.1
    assert _flagged(BOXBOX, q, o)
    o = out.copy()
    o[1:4] += 1e-9 * np.array([1.0, 0, 0])
    assert _flagged(BOXBOX, q, o)
    # a first point in place of the stretch end
    q = _case(CAPBOX, f"tilted by 0.1 deg h={nc.BOARD}/posed")
    out = run(CAPBOX, q)
    assert out[7] == 1 and not _flagged(CAPBOX, q, out)
    far = int(np.argmax([np.linalg.norm(out[8 + 6 * e:11 + 6 * e] - out[1:4]) for e in range(2)]))
    o = out.copy()
    o[8 + 6 * far:11 + 6 * far], o[11 + 6 * far:14 + 6 * far] = out[1:4], out[4:7]
    assert _flagged(CAPBOX, q, o)
    o = out.copy()
    o[11:14] += 1e-9 * np.array([0, 0, 1.0])       # ... a box point that is not the clamp of its axis point
    assert _flagged(CAPBOX, q, o)
    # a wrong answer where the sampled rule decides with its margin
    o = out.copy()
    o[7:20] = 0
    assert _flagged(CAPBOX, q, o)
