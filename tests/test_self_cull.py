"""The broadphase of collide's robot - robot round (self_near, csrc/hrgym_kernels.h) as a statement about geometry, without a GPU: the bound of
tests/self_cull_ref.py -- the longer capsule of a pair as a segment, the shorter one as its bounding sphere, 1e-9 m of slack -- against the exact distance of the two
axis segments (tests/narrowphase_ref.py) on 6144 seeded postures uniform in the joint limits (the first 4096 hold too few near misses for the counts below).

A pair is a contact when its exact distance is below r_i + r_j; no such pair may be culled.  The sample has to put that to the test: counted on the reference alone,
at least 40 postures hold a penetrating pair and at least 40 hold a pair whose surfaces are less than 5 mm apart.  tests/test_self_cull_gpu.py runs the same postures
through the kernels."""
import numpy as np

from narrowphase_ref import seg_seg_ref
from self_cull_ref import LEN2_MIN, N_POSTURES, bound_near, sample

NEAR_MISS = 5e-3   # metres


def test_vectorised_distance_is_the_exact_reference():
    """segment_distance against seg_seg_ref, one pair per call: every pair of the sample within 2 cm of contact and a random tenth of the rest.  1e-12 m: both take
    the minimum over the same candidates in float64, at lengths below 2 m (narrowphase_ref.TOL)"""
    _, M, _, caps, dist = sample()
    gap = dist - M["rsum"]
    pick = (gap < 0.02) | (np.random.RandomState(1).uniform(size=gap.shape) < 0.1)
    assert (gap < 0.02).sum() >= 100
    worst = 0.0
    for k, p in zip(*np.nonzero(pick)):
        i, j = M["ij"][p]
        worst = max(worst, abs(seg_seg_ref(caps[k, i, 0:3], caps[k, i, 3:6], caps[k, j, 0:3], caps[k, j, 3:6])["d"] - dist[k, p]))
    print(f"{int(pick.sum())} pairs, max abs difference {worst:.3e}")
    assert worst <= 1e-12


def test_sample_exercises_the_decision():
    _, M, q, _, dist = sample()
    gap = dist - M["rsum"]
    penetrating = (gap < 0).any(axis=1)
    near_miss = ((gap >= 0) & (gap < NEAR_MISS)).any(axis=1)
    print(f"{len(q)} postures: {int(penetrating.sum())} with a penetrating pair, {int(near_miss.sum())} with a pair separated by less than {NEAR_MISS} m")
    assert len(q) == N_POSTURES
    assert penetrating.sum() >= 40
    assert near_miss.sum() >= 40


def test_degenerate_pairs_are_candidates():
    """a pair of two capsules of length 0 is among the candidates (the closest point of its "segment" is p1), and so are pairs with one such capsule"""
    _, M, _, _, _ = sample()
    point = M["len2"] <= LEN2_MIN
    i, j = M["ij"][:, 0], M["ij"][:, 1]
    assert (point[i] & point[j]).any()
    assert (point[i] ^ point[j]).any()
    assert (M["inv_len2"][point[M["s"]]] == 0).all() and (M["inv_len2"][~point[M["s"]]] > 0).all()
    assert (M["len2"][M["s"]] >= M["len2"][M["o"]]).all()


def test_no_contact_is_culled():
    _, M, _, caps, dist = sample()
    near = bound_near(M, caps)
    contact = dist < M["rsum"]
    print(f"pairs that pass per posture: {near.sum() / len(caps):.3f}; contacts per posture: {contact.sum() / len(caps):.3f}")
    assert not (contact & ~near).any()
    # the margin the bound keeps: the smallest exact surface gap among the culled pairs
    assert (dist - M["rsum"])[~near].min() > 0
    assert (~near).sum() > 0.9 * near.size   # ... and it does cull
