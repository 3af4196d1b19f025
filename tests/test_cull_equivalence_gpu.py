"""The culls of collide and shield_step (cull_box, csrc/hrgym_device.h) inside the stepper: 64 envs, SSM shield, horizon 100, 200 policy steps side by side with the
oracle through tests/parity.py at that helper's tolerances, the HIP state re-synchronised to the oracle's after every step.  -m gpu.

A wrong cull box drops or adds a robot - human pair (collide: `ncon`, `con_pairs`) or a reach-capsule test (shield_step: `is_safe`), so these three must equal the
oracle's exactly in every step.  The run has to exercise both culls: counted on the oracle alone, at least 20 env-steps list a robot - human contact pair and at
least 20 carry a fail-safe intervention; both counts are asserted.  The human is placed with human_rand = [0.6, 0.6, 0.5] so that it walks into the arm's reach
(without it the synthetic clips never touch the robot in 200 steps; counted on the oracle: 194 / 2196 env-steps with a contact pair / an intervention for
ReachHuman, 225 / 2429 with robot_geometry="hull", 319 / 4534 for PickPlaceHumanCart)."""
import numpy as np
import pytest

from human_robot_gym_amd._cstruct import CONST, EnvState
from helpers import compare_states_bulk, make_pair, states_as_bytes
from parity import Run

pytestmark = pytest.mark.gpu
REPRESENTATIONS = ("ltt.dur", "ltt.jerk", "safe_path.dur", "safe_path.jerk")   # segment tables: compared through the motion they command (helpers.assert_state_close)

N_ENVS, N_STEPS, SEED = 64, 200, 1
KW = dict(shield_type="SSM", reward_shaping=True, horizon=100, human_rand=[0.6, 0.6, 0.5])
NR, NHB = CONST["HRG_NRCAP"], CONST["HRG_NHB"]   # geoms: robot capsules, then the human's bodies


def _ints(st, name):
    """one int32 field of every env state: [n]"""
    f = getattr(EnvState, name)
    return np.ascontiguousarray(states_as_bytes(st)[:, f.offset:f.offset + 4]).view(np.int32)[:, 0].copy()


def rollout(name, second=None, **desc_kw):
    """(env-steps with a robot - human contact pair, env-steps with a fail-safe intervention) on the oracle, after holding the second side to it in every step"""
    task = dict(task_frames=(300, 600)) if "env_id" in desc_kw else {}
    O, G = make_pair(N_ENVS, KW, second=second, **task, **desc_kw)
    run = Run(O, G, f"test_cull_equivalence_gpu::{name}")
    rng = np.random.RandomState(SEED)
    n_contact = n_failsafe = 0
    for s in run.steps(N_STEPS, lambda k: rng.uniform(-1, 1, (N_ENVS, 7))):
        # the state blocks: every integer exactly and every float at the harness's tolerances in every step (helpers.compare_states_bulk, all envs at once); the
        # harness's own env-by-env comparison, which also samples the trajectories that the segment tables stand for, costs 0.4 s per step at 64 envs and runs on
        # every tenth step and the last
        full = s.k % 10 == 0 or s.k == N_STEPS - 1
        s.compare(skip=() if full else ("state",))
        if not full:
            for so, sg, skip in ((s.o.states, s.g.states, REPRESENTATIONS), (s.o.objects, s.g.objects, ())):
                if so is not None:
                    ok, msg = compare_states_bulk(so, sg, skip=skip)
                    assert ok[s.chk].all(), f"{s.msg}: state differs in envs {np.flatnonzero(~ok & s.chk).tolist()} (first mismatch of the batch: {msg})"
        for what, got, want in (("ncon", s.g.ncon, s.o.ncon), ("con_pairs", s.g.pairs, s.o.pairs), ("is_safe", _ints(s.g.states, "is_safe"), _ints(s.o.states, "is_safe"))):
            bad = (got != want).reshape(N_ENVS, -1).any(axis=1) & s.chk
            assert not bad.any(), f"{s.msg}: {what} differs in envs {np.flatnonzero(bad).tolist()}"
        listed = np.arange(s.o.pairs.shape[1])[None, :] < s.o.ncon[:, None]
        robot_human = listed & (s.o.pairs[:, :, 0] < NR) & (s.o.pairs[:, :, 1] >= NR) & (s.o.pairs[:, :, 1] < NR + NHB)
        n_contact += int(robot_human.any(axis=1).sum())
        n_failsafe += int((_ints(s.o.states, "failsafe_interventions") > _ints(s.pre_states, "failsafe_interventions")).sum())   # (the counter of the episode: at most +1 per step)
        s.resync()
    compared = run.compared
    run.finish()
    print(f"[cull] {name}: {n_contact} env-steps with a robot-human pair, {n_failsafe} with a fail-safe intervention, {compared} of {N_ENVS * N_STEPS} env-steps compared")
    assert compared >= 0.9 * N_ENVS * N_STEPS
    return n_contact, n_failsafe


@pytest.mark.parametrize("name,desc_kw", [("ReachHuman", {}), ("ReachHuman_hull", dict(robot_geometry="hull")), ("PickPlaceHumanCart", dict(env_id="PickPlaceHumanCart"))])
def test_culls_keep_contacts_and_verdicts(name, desc_kw):
    n_contact, n_failsafe = rollout(name, **desc_kw)
    assert n_contact >= 20, "the run was meant to bring the human into contact with the arm"
    assert n_failsafe >= 20, "the run was meant to trigger the shield"
