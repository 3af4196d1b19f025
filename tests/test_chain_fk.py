"""The numpy chain of tests/chain_fk_ref.py against what the CPU oracle exports (no GPU): the end effector position of its robot kinematics, at a reset batch's
state and at arbitrary angles, and the robot reach capsules its shield reports.  tests/test_chain_fk_gpu.py measures the kernels' chain walk with that numpy chain,
so it has to be pinned first.

Tolerance 1e-12 absolute: every entry is a sum of fewer than 200 products of magnitude at most 1.5 (metres, or rotation entries), so the rounding error of either
side is below 200 * 1.5 * 2^-53 = 3e-14."""
import ctypes

import numpy as np
import pytest

import human_robot_gym_amd as hrg
from human_robot_gym_amd._cstruct import CONST

from chain_fk_ref import NARM, NCAP, NV, chain

ATOL = 1e-12


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _oracle_eef(lib, d, q):
    M, b, eef = np.zeros((NV, NV)), np.zeros(NV), np.zeros(3)
    lib.hrgo_test_robot(ctypes.byref(d), _p(np.ascontiguousarray(q)), _p(np.zeros(NV)), _p(M), _p(b), _p(eef))
    return eef


def _eef(d, R, p):
    return p[NARM - 1] + R[NARM - 1] @ np.array(list(d.eef_pos))


def test_rotations_are_rotations():
    d = hrg.build_model_desc()
    R, _, _ = chain(d, np.linspace(-1.5, 1.5, NARM))
    for i in range(NV):
        np.testing.assert_allclose(R[i] @ R[i].T, np.eye(3), atol=1e-14)
        assert abs(np.linalg.det(R[i]) - 1) < 1e-14


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_end_effector_is_the_oracles(oracle_lib, seed):
    d = hrg.build_model_desc()
    lo, hi = (np.array(list(d.qpos_limits[k]))[:NARM] for k in (0, 1))
    rng = np.random.RandomState(seed)
    qs = [rng.uniform(lo, hi) for _ in range(8)] + [np.zeros(NARM), lo, hi, np.full(NARM, np.pi / 2), np.full(NARM, -np.pi / 4)]
    for q in qs:
        R, p, _ = chain(d, q)
        np.testing.assert_allclose(_eef(d, R, p), _oracle_eef(oracle_lib, d, np.concatenate([q, np.zeros(NV - NARM)])), rtol=0, atol=ATOL)


def test_reset_batch_end_effector_and_reach_capsules_are_the_oracles(oracle_lib):
    """a reset batch, then one policy step with the zero action: the goal is the configuration the robot is in, so the shield's current configuration and the one
    at the end of its brake are both that configuration and each reported reach capsule (the mid points of the two) has the chain's own end points"""
    from oracle.oracle import OracleBatch
    n = 4
    clips = hrg.synthetic_clips(2, seed=0, min_frames=300, max_frames=400)
    d = hrg.build_model_desc(dict(shield_type="SSM"), n_clips=clips.n_clips)
    O = OracleBatch(d, clips, n)
    try:
        O.reset()
        q0 = []
        for e in range(n):
            s = O.get_state(e)
            q = np.array(list(s.qpos))
            R, p, _ = chain(d, q[:NARM], q[NARM:])
            np.testing.assert_allclose(np.array(list(s.eef_pos)), _eef(d, R, p), rtol=0, atol=ATOL)
            q0.append(q[:NARM])
        O.step(np.zeros((n, CONST["HRG_ACT_DIM"])))
        rcap, _, _ = O.capsules()
        for e in range(n):
            s = O.get_state(e)
            np.testing.assert_allclose(np.array(list(s.des_q))[:NARM], q0[e], rtol=0, atol=1e-15)   # the commanded configuration has not moved
            _, _, caps = chain(d, q0[e])
            assert rcap.shape[1:] == (NCAP, 7)
            np.testing.assert_allclose(rcap[e, :, :6], caps, rtol=0, atol=ATOL)
    finally:
        O.close()
