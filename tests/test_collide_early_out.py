"""The plane verdict behind collide's early-out (csrc/hrgym_kernels.h) as a statement about the capsules, without a GPU.

Before its pair rounds collide takes three broadphase verdicts; when no robot self pair comes near, no human capsule is listed and the PLANES ARE CLEAR it skips the
rounds as a whole.  "Clear": zmin >= table_top_z and zmin >= floor_z, with zmin the minimum of p[2] - rcap_r[i] over both end points p of every capsule that moves
(rcap_body[i] >= 0; the plane round leaves the capsules of the base out as well).  The plane round reports end point p of capsule i against
the plane at z0 only when p[2] - rcap_r[i] - z0 < 0 (and, for the table, when p lies over the slab), so a substep whose planes are clear holds no plane contact:
x >= y implies x - y >= 0 in IEEE arithmetic, and zmin is the smallest p[2] - rcap_r[i] of the round's own end points.

Here: the 6144 seeded postures of tests/self_cull_ref.py with that file's kinematics.  Wherever the verdict says clear, no end point satisfies the round's hit
condition, written out as the round evaluates it.  The kernels reduce zmin as a maximum of negated values (cull_box: max(-z1, -z2) + r per capsule, the maximum over
the capsules, negated); that route gives the double of the plain minimum, bit for bit.  The sample holds postures of both kinds -- counted on the numpy side alone,
5238 are clear and 906 are not, 733 of those with an end point the round reports (all against the table; none reaches the floor) -- and the verdict is no wider
than it has to be: a posture that is not clear has a moving end point below the higher of the two planes.  tests/test_collide_early_out_gpu.py runs postures of
both kinds through the steppers."""
import numpy as np

from self_cull_ref import N_POSTURES, sample

SLAB_MID = 0.025   # metres below the table top: the mid-plane of the 0.05 m slab, below which an end point is not the table's


def planes(desc, M, caps):
    """(clear [n], hit_table [n][NRCAP][2], hit_floor [n][NRCAP][2], low [n][NRCAP][2]) of capsules caps [n][NRCAP][6]; low = p[2] - r per end point"""
    moves = M["body"] >= 0
    P = caps.reshape(len(caps), -1, 2, 3)
    low = P[..., 2] - M["r"][None, :, None]
    zmin = np.where(moves[None, :, None], low, np.inf).min(axis=(1, 2))
    clear = (zmin >= desc.table_top_z) & (zmin >= desc.floor_z)
    over = (np.abs(P[..., 0] - desc.table_center[0]) <= desc.table_half[0]) & (np.abs(P[..., 1] - desc.table_center[1]) <= desc.table_half[1]) & (P[..., 2] > desc.table_top_z - SLAB_MID)
    hit_table = moves[None, :, None] & over & (low - desc.table_top_z < 0)
    hit_floor = moves[None, :, None] & (low - desc.floor_z < 0)
    return clear, hit_table, hit_floor, low


def test_a_clear_verdict_leaves_no_plane_contact():
    desc, M, q, caps, _ = sample()
    clear, hit_table, hit_floor, low = planes(desc, M, caps)
    hit = (hit_table | hit_floor).any(axis=(1, 2))
    print(f"{len(q)} postures: {int(clear.sum())} clear, {int((~clear).sum())} not clear, {int(hit.sum())} with a plane contact "
          f"({int(hit_table.any(axis=(1, 2)).sum())} table, {int(hit_floor.any(axis=(1, 2)).sum())} floor)")
    assert len(q) == N_POSTURES
    assert not (clear & hit).any()
    # both kinds, and contacts for the verdict to let through
    assert clear.sum() >= 1000 and (~clear).sum() >= 500 and hit.sum() >= 400
    # no wider than it has to be: not clear <=> a moving end point is below the higher plane
    moves = M["body"] >= 0
    below = (moves[None, :, None] & (low < max(desc.table_top_z, desc.floor_z))).any(axis=(1, 2))
    assert np.array_equal(~clear, below)
    assert (~moves).any()   # the model has a capsule of the base, which round and verdict both leave out


def test_negated_maximum_is_the_minimum():
    """cull_box's route to zmin: per capsule max(-z1, -z2) + r, the maximum over the capsules that move, negated"""
    _, M, _, caps, _ = sample()
    moves = M["body"] >= 0
    z, r = caps[:, moves][:, :, [2, 5]], M["r"][moves]
    direct = (z - r[None, :, None]).min(axis=(1, 2))
    routed = -(np.maximum(-z[..., 0], -z[..., 1]) + r[None, :]).max(axis=1)
    assert np.array_equal(direct.view(np.uint64), routed.view(np.uint64))
