"""The robot - robot round of collide in the kernels against tests/self_cull_ref.py (which tests/test_self_cull.py holds to the exact segment distance).  -m gpu.

hrg_debug_self_pairs runs the chain walk, the capsule end points and the round for one posture per wavefront, as the batch's kernel variant compiles them, and reports
per candidate pair the broadphase verdict, the contact of the round and the contact of the narrowphase with the broadphase compiled out.  On the 6144 postures of
the CPU test, for the ReachHuman kernels and for a cube variant (another LDS image, the same functions):
  - a culled pair never has a reference distance below r_i + r_j;
  - the contacts with the cull equal those without it bit for bit;
  - every penetrating pair of the reference is reported, and nothing is reported that the reference holds clear.
"Penetrating" and "clear" leave a band of EDGE = 1e-10 m around r_i + r_j to the rounding: the kernels' capsule end points are within CHAIN = 1e-12 m of the numpy
chain's (tests/test_chain_fk_gpu.py; asserted here as well), so the two segment distances differ by at most 4e-12 m and seg_seg's own error at these lengths is
below 1e-12 (tests/test_narrowphase_gpu.py).

Then the round inside the stepper, in the style of tests/test_cull_equivalence_gpu.py: 64 envs moved through the state I/O to postures in self-contact, 5 policy
steps side by side with the oracle, which enumerates every pair: `ncon` and `con_pairs` equal the oracle's in every step, and counted on the oracle alone at least
20 envs list a robot - robot pair."""
import ctypes

import numpy as np
import pytest

from human_robot_gym_amd._cstruct import CONST, EnvState

from self_cull_ref import NRCAP, sample

pytestmark = pytest.mark.gpu

CHAIN, EDGE = 1e-12, 1e-10
NARM = CONST["HRG_NARM"]
SP_MAX, SP_DIM, SP_PAIRS, SP_PDIM, SP_NPAIR = (CONST[k] for k in ("HRG_SP_MAX", "HRG_SP_DIM", "HRG_SP_PAIRS", "HRG_SP_PDIM", "HRG_SP_NPAIR"))


@pytest.fixture(scope="module", params=["ReachHuman", "PickPlaceHumanCart"])
def tapped(request):
    """(model, caps, dist) of the reference and the tap's output (caps [n][NRCAP][6], pairs [n][SP_NPAIR][SP_PDIM]) for the variant's own model, computed once"""
    import human_robot_gym_amd as hrg
    from human_robot_gym_amd._lib import HipBatch
    from human_robot_gym_amd.mixed import task_clips
    env_id = request.param
    desc, M, q, caps, dist = sample(env_id)
    clips = task_clips(env_id, 2, min_frames=300, max_frames=400)
    G = HipBatch(desc, clips, 2)
    out = np.full((len(q), SP_DIM), np.nan)
    for k0 in range(0, len(q), SP_MAX):
        qk, ok = np.ascontiguousarray(q[k0:k0 + SP_MAX]), out[k0:k0 + SP_MAX]
        rc = G.lib.hrg_debug_self_pairs(G.h, qk.ctypes.data_as(ctypes.c_void_p), len(qk), ok.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0, G.lib.hrg_last_error().decode()
    big = np.zeros((SP_MAX + 1, NARM))
    assert G.lib.hrg_debug_self_pairs(G.h, big.ctypes.data_as(ctypes.c_void_p), SP_MAX + 1, out.ctypes.data_as(ctypes.c_void_p)) != 0   # more than a launch
    G.close()
    assert np.isfinite(out).all()
    return M, caps, dist, out[:, :SP_PAIRS].reshape(len(q), NRCAP, 6), out[:, SP_PAIRS:].reshape(len(q), SP_NPAIR, SP_PDIM)


def test_tap_walks_the_reference_postures(tapped):
    M, caps, _, gcaps, gp = tapped
    npair = len(M["ij"])
    worst = np.abs(gcaps - caps).max()
    print(f"capsule end points: max abs difference {worst:.3e}")
    assert worst <= CHAIN
    assert (gp[:, :npair, 0:2] == M["ij"][None]).all()   # the pairs in enumeration order
    assert (gp[:, npair:] == 0).all()


def test_culled_pairs_are_clear_and_contacts_unchanged(tapped):
    M, _, dist, _, gp = tapped
    npair = len(M["ij"])
    near, on, off = gp[:, :npair, 2] != 0, gp[:, :npair, 3:11], gp[:, :npair, 11:19]
    gap = dist - M["rsum"]
    print(f"pairs that pass per posture {near.sum() / len(gp):.3f}; contacts reported {int((on[..., 0] != 0).sum())}; "
          f"smallest reference gap of a culled pair {gap[~near].min():.3e} m")
    assert not (~near & (gap < 0)).any()
    assert np.array_equal(np.ascontiguousarray(on).view(np.uint64), np.ascontiguousarray(off).view(np.uint64))
    assert near.sum() < 0.2 * len(gp)   # the cull is compiled in: bounding spheres alone pass more than two pairs per posture
    hit = on[..., 0] != 0
    assert hit[gap < -EDGE].all()
    assert not hit[gap > EDGE].any()
    assert (hit <= near).all()
    # what a reported contact says: its distance is the reference's
    assert np.abs(on[..., 1][hit] - gap[hit]).max() <= EDGE


N_ENVS, N_STEPS = 64, 5
KW = dict(shield_type="SSM", reward_shaping=True, horizon=100)


def robot_robot(pairs, ncon):
    """[n] bool: the env's contact list holds a pair of two robot capsules"""
    listed = np.arange(pairs.shape[1])[None, :] < ncon[:, None]
    return (listed & (pairs[:, :, 0] < NRCAP) & (pairs[:, :, 1] < NRCAP)).any(axis=1)


def self_contact_postures():
    """N_ENVS postures that the oracle alone shows in self-contact: the sample's postures with a penetrating pair, placed on a batch of the oracle's and stepped once
    (the arm is pushed apart during the step, and an episode that ends is reset: fewer than half still list the pair afterwards); those that do, repeated to N_ENVS"""
    import human_robot_gym_amd as hrg
    from oracle.oracle import OracleBatch
    _, M, q, _, dist = sample()
    cand = q[(dist < M["rsum"]).any(axis=1)]
    clips = hrg.synthetic_clips(3, seed=0, min_frames=300, max_frames=600)
    O = OracleBatch(hrg.build_model_desc(dict(KW), n_clips=clips.n_clips), clips, len(cand), 0)
    O.reset()
    place(O, cand)
    O.step(np.zeros((len(cand), 7)))
    keep = robot_robot(*O.contacts()) & ~np.asarray(O.done, bool)
    O.close()
    assert keep.sum() >= 20
    return cand[np.resize(np.flatnonzero(keep), N_ENVS)]


def place(B, q):
    """move every env of a freshly reset batch to q, at rest, its shield state as after a reset there (tests/shield_scenarios.py: Scenario.place)"""
    from parity import read_blocks, write_blocks
    from shield_audit import states_array
    s = states_array(read_blocks(B, None)[0])
    s["qpos"][:, :NARM] = q
    s["qpos"][:, NARM:] = 0.0   # (fingers: a reset scatters them per env)
    s["qvel"][:] = 0.0
    s["qacc_warmstart"][:] = 0.0
    for f in ("goal_qpos", "new_goal_q", "des_q", "cur_goal"):
        s[f][:] = q
    s["ltt"]["q0"][:] = q
    s["ltt"]["qT"][:] = q
    write_blocks(B, None, (EnvState * len(s)).from_buffer_copy(s.tobytes()), None)


def stepper_run(second=None):
    """envs of the first step that list a robot - robot pair on the oracle, after holding the second side's contact lists to the oracle's in every step"""
    from helpers import make_pair
    from parity import Run, read_blocks, write_blocks
    O, G = make_pair(N_ENVS, KW, second=second)
    run = Run(O, G, "test_self_cull_gpu::stepper")
    place(O, self_contact_postures())
    write_blocks(G, None, *read_blocks(O, None))
    listed_first = None
    for s in run.steps(N_STEPS, lambda k: np.zeros((N_ENVS, 7))):
        s.compare()
        for what, got, want in (("ncon", s.g.ncon, s.o.ncon), ("con_pairs", s.g.pairs, s.o.pairs)):
            bad = (got != want).reshape(N_ENVS, -1).any(axis=1) & s.chk
            assert not bad.any(), f"{s.msg}: {what} differs in envs {np.flatnonzero(bad).tolist()}"
        n_listed = int((robot_robot(s.o.pairs, s.o.ncon) & s.chk).sum())   # (s.chk: the harness leaves out an env whose step was violent, |qvel| > 5 rad/s)
        print(f"{s.msg}: {n_listed} envs list a robot-robot pair, {int(s.chk.sum())} envs compared in full")
        if listed_first is None:
            listed_first = n_listed
        s.resync()
    run.finish()
    return listed_first


def test_stepper_lists_the_oracles_self_contacts():
    assert stepper_run() >= 20, "the postures were meant to put the arm into contact with itself"
