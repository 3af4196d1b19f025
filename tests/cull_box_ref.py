"""Reference of cull_box (csrc/hrgym_device.h): the box around up to 16 capsules, each inflated by its radius, that collide and shield_step cull against.

The device spreads the six bounds over the wave: lane l serves capsule c = l & 15 and quantity g = l >> 4.  The first row maximum carries hi_x, -lo_x, hi_y, -lo_y in the
DPP rows 0..3, the second hi_z, -lo_z in rows 0, 1 (rows 2, 3 idle); a lane without a capsule holds EMPTY.  `box_by_lanes` restates that layout lane by lane,
`box_numpy` is numpy's min and max over the capsules: tests/test_cull_box.py holds the two together on the CPU, tests/test_cull_box_gpu.py the device against numpy."""
import numpy as np

EMPTY = -1e300
NS = (1, 7, 10, 16)                     # 7: the shield's reach capsules, 10: the robot's collision capsules, 16: a full row
# (axis, negated) of quantity g in the first and in the second reduction; None: the row is idle
PASS1 = ((0, False), (0, True), (1, False), (1, True))
PASS2 = ((2, False), (2, True), None, None)


def lane_role(lane, n):
    """(capsule, role in the first reduction, role in the second) of a lane; capsule None: the lane has none and holds EMPTY in both"""
    c, g = lane & 15, lane >> 4
    return (c if c < n else None), PASS1[g], PASS2[g]


def _bound(cap, role):
    axis, neg = role
    p1, p2, r = cap[axis], cap[3 + axis], cap[6]
    return max(-p1, -p2) + r if neg else max(p1, p2) + r


def lane_values(caps, n):
    """(e1[64], e2[64]): what every lane holds going into the two row maxima"""
    e = np.full((2, 64), EMPTY)
    for lane in range(64):
        c, r1, r2 = lane_role(lane, n)
        if c is not None:
            e[0, lane] = _bound(caps[c], r1)
            if r2 is not None:
                e[1, lane] = _bound(caps[c], r2)
    return e[0], e[1]


def box_by_lanes(caps, n):
    """(lo[3], hi[3]) through the lane layout: row maxima, read from the first lane of the rows"""
    e1, e2 = lane_values(np.asarray(caps, np.float64), n)
    m1, m2 = e1.reshape(4, 16).max(axis=1), e2.reshape(4, 16).max(axis=1)
    return np.array([-m1[1], -m1[3], -m2[1]]), np.array([m1[0], m1[2], m2[0]])


def box_numpy(caps, n):
    """(lo[3], hi[3]) as numpy's min and max over the first n capsules"""
    c = np.asarray(caps, np.float64)[:n]
    p1, p2, r = c[:, 0:3], c[:, 3:6], c[:, 6:7]
    return (np.minimum(p1, p2) - r).min(axis=0), (np.maximum(p1, p2) + r).max(axis=0)


def cases():
    """{name: caps[16][7]}: p1[3] p2[3] r per capsule"""
    rng = np.random.RandomState(19)
    out = {}
    c = rng.uniform(-2, 2, (16, 7)); c[:, 6] = rng.uniform(0.01, 0.3, 16)
    out["random"] = c
    c = rng.uniform(-2, 2, (16, 7)); c[:, 3:6] = c[:, 0:3]; c[:, 6] = rng.uniform(0.0, 0.2, 16); c[::3, 6] = 0.0
    out["degenerate"] = c                                       # p1 = p2, every third one a point
    c = np.zeros((16, 7)); c[::2, 0:3] = -0.0; c[1::4, 3:6] = -0.0; c[:, 6] = 0.0
    c[5] = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0]
    out["zeros"] = c                                            # +0.0 and -0.0 coordinates, zero radius: every bound is a zero
    c = rng.uniform(-1, 1, (16, 7)); c[:, 6] = 0.05
    c[:, 0] = np.where(np.arange(16) % 2 == 0, 0.0, -0.0); c[:, 4] = np.where(np.arange(16) % 3 == 0, -0.0, 0.0)
    out["zeros_mixed"] = c                                      # zeros of either sign next to ordinary coordinates
    c = rng.uniform(-1, 1, (16, 7)) * 1e-300; c[:, 6] = 1e-300
    out["tiny"] = c                                             # extents of 1e-300
    c = rng.uniform(-1, 1, (16, 7)) * 1e300; c[:, 6] = np.where(np.arange(16) % 2 == 0, 1e300, 1e-300)
    c[0] = [1e300, -1e300, 1e-300, -1e-300, 1e300, -1e300, 1e300]
    out["huge"] = c                                             # extents of 1e+300 (a bound reaches 2e300), next to 1e-300
    c = rng.uniform(-2, 2, (16, 7)); c[:, 6] = 0.1
    c[:, 0:3] -= 50.0; c[:, 3:6] -= 50.0
    out["one_sided"] = c                                        # every bound negative
    return out
