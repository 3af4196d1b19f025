"""HIP stepper vs CPU oracle on identical seeded inputs (through the C ABI).  -m gpu."""
import numpy as np
import pytest

from helpers import make_pair
from parity import Run

pytestmark = pytest.mark.gpu


def _rollout(kw, n_envs, n_steps, seed, resync, clips=None, action_fn=None, min_live=0.9, name=""):
    """Step oracle and HIP side by side.  An env whose oracle trajectory turns violent (|qvel| > 5 rad/s before or after the step, e.g. after a
    deep human-robot penetration, or a simulation crash) is chaotic: bit-level agreement of later event counters is
    not a meaningful expectation, so in free-running mode such an env is dropped from then on (counted, bounded)."""
    O, G = make_pair(n_envs, kw, clips=clips)
    run = Run(O, G, f"test_parity_gpu::{name or kw.get('shield_type')}{'' if resync else '_free'}", free_running=not resync, violent="base+pre")
    rng = np.random.RandomState(seed)
    n_coll = 0

    def actions(k):
        a = rng.uniform(-1, 1, (n_envs, 7))
        return a if action_fn is None else action_fn(k, a)
    for s in run.steps(n_steps, actions):
        s.compare()
        n_coll += int(s.o.info[s.chk][:, 0].sum())
        if resync:
            s.resync()
    run.finish(min_live)
    return n_coll


@pytest.mark.parametrize("shield", ["OFF", "SSM"])
def test_step_parity_resync(shield):
    """Per-step parity with the GPU state re-synchronised to the oracle after every step."""
    kw = dict(shield_type=shield, reward_shaping=True, horizon=20)
    _rollout(kw, n_envs=16, n_steps=45, seed=1, resync=True)


@pytest.mark.parametrize("shield", ["OFF", "SSM"])
def test_step_parity_free_running(shield):
    """Free-running rollouts (no resync) incl. auto-resets: trajectories stay within tolerance."""
    kw = dict(shield_type=shield, reward_shaping=True, human_rand=[0.3, 0.3, 0.5], horizon=15)
    _rollout(kw, n_envs=32, n_steps=40, seed=2, resync=False)


def test_contacts_and_collisions_occur():
    """A T-pose human whose hand is 0.3 m from the upright arm; the shoulder joint is driven into it: contacts are
    generated, enter the constraint solve, are classified, and all of it agrees with the oracle."""
    import human_robot_gym_amd as hrg
    clips = hrg.static_clip(600, pelvis=(-0.8, 1.0, 0.3))
    for c in clips.infos:
        c["position_offset"] = [0.0, 0.0, 0.0]
    kw = dict(shield_type="OFF", horizon=30, done_at_collision=False, collision_reward=-10)

    def act(k, a):
        a[:, 1] = np.where(np.arange(len(a)) % 2 == 0, 1.0, -1.0)  # tilt the arm towards / away from the hand
        a[:, [0, 2, 3, 4, 5]] *= 0.2
        return a
    n_coll = _rollout(kw, n_envs=16, n_steps=22, seed=5, resync=True, clips=clips, action_fn=act, min_live=0.75, name="contacts")   # (measured: 16 of 16)
    assert n_coll > 0, "scenario was meant to produce collisions"
