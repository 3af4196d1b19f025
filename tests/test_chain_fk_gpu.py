"""robot_chain_fk on its own (hrg_debug_chain_fk: one wave per triple of configurations) against the numpy chain of tests/chain_fk_ref.py, which
tests/test_chain_fk.py pins to the oracle.  -m gpu.

The walk reads the first two columns of every joint's rotation from a table that 18 lanes fill ahead of it, and runs unrolled from per-lane base addresses: the
cases are the angles at which the sine / cosine code changes its path (sincos_small reduces by pi/2: the quadrant changes at odd multiples of pi/4, the sign pattern at
multiples of pi/2), the joint limits, zeros and seeded random vectors, with and without the shield (without it only the simulation state is walked), for the
ReachHuman kernels and for a cube variant, which compile the same function against another LDS image.

Tolerance 1e-12 absolute: every entry is a sum of fewer than 200 products of magnitude at most 1.5 (metres, or rotation entries), so its rounding error is below
200 * 1.5 * 2^-53 = 3e-14; 1e-12 is thirty times that bound."""
import ctypes

import numpy as np
import pytest

import human_robot_gym_amd as hrg

from chain_fk_ref import NARM, chain, tap_layout
from human_robot_gym_amd._cstruct import CONST

pytestmark = pytest.mark.gpu

ATOL = 1e-12


def _special(lo, hi):
    """[n][3][NARM]: zeros, both joint limits, and every multiple of pi/4 up to +-pi with its two neighbouring doubles, the same angle in every joint; the three
    configurations of a triple take consecutive rows of that list, so each differs from the other two"""
    vals = [np.zeros(NARM), lo, hi]
    for k in range(-4, 5):
        x = k * np.pi / 4
        vals += [np.full(NARM, v) for v in (np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf))]
    vals = np.array(vals)
    return np.stack([vals, np.roll(vals, 1, axis=0), np.roll(vals, 2, axis=0)], axis=1)


def _random(lo, hi):
    rng = np.random.RandomState(20)
    return rng.uniform(lo, hi, (50, 3, NARM))


CASES = {"special": _special, "random": _random}


@pytest.fixture(scope="module", params=["ReachHuman", "PickPlaceHumanCart"])
def batch(request):
    from human_robot_gym_amd._lib import HipBatch
    from human_robot_gym_amd.mixed import task_clips, task_env_kwargs
    env_id = request.param
    clips = task_clips(env_id, 2, min_frames=300, max_frames=400)
    desc = hrg.build_model_desc(dict(task_env_kwargs(env_id)), n_clips=clips.n_clips, env_id=env_id)
    G = HipBatch(desc, clips, 2)
    yield G, desc, env_id
    G.close()


_REF = {}


def _reference(env_id, desc, case, q):
    """the numpy chain of every configuration of the case for the model of `env_id`, computed once and shared by the tests"""
    if (env_id, case) not in _REF:
        _REF[env_id, case] = [[chain(desc, q[k, c]) for c in range(3)] for k in range(len(q))]
    return _REF[env_id, case]


@pytest.mark.parametrize("shield_on", [True, False])
@pytest.mark.parametrize("case", sorted(CASES))
def test_chain_walk_is_the_numpy_chain(batch, case, shield_on):
    G, desc, env_id = batch
    lo, hi = (np.array(list(desc.qpos_limits[k]))[:NARM] for k in (0, 1))
    q = np.ascontiguousarray(CASES[case](lo, hi))
    n = len(q)
    assert n <= 64
    out = np.full((n, CONST["HRG_CFK_DIM"]), np.nan)
    rc = G.lib.hrg_debug_chain_fk(G.h, q.ctypes.data_as(ctypes.c_void_p), n, int(shield_on), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, G.lib.hrg_last_error().decode()
    kR, kp, scap = tap_layout(out)
    ref = _reference(env_id, desc, case, q)
    worst = 0.0
    for k in range(n):
        R, p, _ = ref[k][2]
        worst = max(worst, np.abs(kR[k] - R).max(), np.abs(kp[k] - p).max())
        if shield_on:   # without the shield the first two configurations are not walked: their block is not read
            for c in range(2):
                worst = max(worst, np.abs(scap[k, c] - ref[k][c][2]).max())
    print(f"{case} shield_on={shield_on}: n={n} max abs difference {worst:.3e}")
    assert np.isfinite(kR).all() and np.isfinite(kp).all()
    assert worst <= ATOL


def test_tap_rejects_more_than_a_launch(batch):
    G = batch[0]
    q = np.zeros((65, 3, NARM))
    out = np.zeros((65, CONST["HRG_CFK_DIM"]))
    assert G.lib.hrg_debug_chain_fk(G.h, q.ctypes.data_as(ctypes.c_void_p), 65, 1, out.ctypes.data_as(ctypes.c_void_p)) != 0
