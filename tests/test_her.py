"""Hindsight experience replay, host side: compute_done on the goal-env interface, the ABI and where its header is compiled, the refusals of attach_her, the
config translation, and self-checks of tests/her_ref.py (the numpy restatement the device is compared with in tests/test_her_gpu.py).  No GPU."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import her_ref as R
import human_robot_gym_amd as hrg
from helpers import OracleBackend
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.env_util import make_vec_env


def _goal_env(env_id, n=6, backend=True, **kw):
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    # goal_dist: random actions move the arm by a few hundredths per step; at these thresholds some envs of seed 6 succeed within the horizon and most do not
    kw = dict(dict(shield_type="OFF", horizon=12, seed=6, goal_dist=3.4 if env_id == "ReachHuman" else 0.6), **kw)
    desc = hrg.build_model_desc(kw, n_clips=clips.n_clips, env_id=env_id)
    return make_vec_env(env_id, type="goal_env", n_envs=n, env_kwargs=kw, vec_env_kwargs=dict(clips=clips, backend=OracleBackend(desc, clips, n) if backend else None))


@pytest.mark.parametrize("env_id", ["ReachHuman", "PickPlaceHumanCart"])
@pytest.mark.parametrize("das", [0, 1])
@pytest.mark.parametrize("dac", [0, 1])
def test_compute_done_is_the_env_rule_and_agrees_with_the_stepped_done(env_id, das, dac):
    """HumanEnv._check_done (human_env.py:835-858) = (done_at_collision and illegal collision) or (done_at_success and success): equal to the done flag of
    every step without its timeouts, for collision_type 0 and 8, and a relabelled goal is a success."""
    env = _goal_env(env_id, done_at_success=bool(das), done_at_collision=bool(dac))
    obs = env.reset()
    rng = np.random.RandomState(0)
    seen = dict(done=0, timeout=0)
    for k in range(14):
        obs, rew, done, infos = env.step(rng.uniform(-1, 1, (6, 7)))
        term = {key: np.stack([infos[i]["terminal_observation"][key] if done[i] else obs[key][i] for i in range(6)]) for key in obs}
        trunc = np.array([bool(i.get("TimeLimit.truncated", False)) for i in infos])
        d2 = env.compute_done(term["achieved_goal"], term["desired_goal"], infos)
        assert d2.dtype == bool and d2.shape == (6,)
        np.testing.assert_array_equal(d2, done & ~trunc, err_msg=f"step {k}")
        seen["done"] += int((done & ~trunc).sum())
        seen["timeout"] += int(trunc.sum())
    assert seen["timeout"] > 0
    if das:
        assert seen["done"] > 0
    ag = term["achieved_goal"]
    relabeled = ag if env_id == "ReachHuman" else ag[:, 3:6]
    for ctype in (0, 8):   # 8: a static collision, illegal
        got = env.compute_done(ag, relabeled, [dict(collision_type=ctype)] * 6)
        assert np.all(got == bool(das or (dac and ctype == 8))), (ctype, got)
        far = relabeled + 2.0   # 2 sqrt(6) or 2 sqrt(3) away: no success
        assert np.all(env.compute_done(ag, far, [dict(collision_type=ctype)] * 6) == bool(dac and ctype == 8))
    one = env.compute_done(ag[0], relabeled[0], dict(collision_type=8))
    assert isinstance(one, bool) and one == bool(das or dac)
    got = env.env_method("compute_done", ag[:2], relabeled[:2], [dict(collision_type=0)] * 2, indices=[0])
    assert len(got) == 1 and got[0].shape == (2,) and np.all(got[0] == bool(das))
    env.close()


def test_compute_done_needs_a_goal_env_and_the_mixed_env_refuses_it():
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    kw = dict(shield_type="OFF", horizon=5)
    env = hrg.HipVecEnv(2, env_kwargs=kw, clips=clips, backend=OracleBackend(hrg.build_model_desc(kw, n_clips=2), clips, 2))
    with pytest.raises(NotImplementedError, match="goal_env"):
        env.compute_done(np.zeros(6), np.zeros(6), dict(collision_type=0))
    with pytest.raises(NotImplementedError, match="goal_env"):
        env.env_method("compute_done", np.zeros(6), np.zeros(6), dict(collision_type=0))
    with pytest.raises(NotImplementedError, match="goal_env"):
        env.attach_her(32)
    env.close()
    stub = NS(step_async=None, env_ids=["ReachHuman", "PickPlaceHumanCart"], slices=[slice(0, 2), slice(2, 4)])
    mixed = hrg.MixedHipVecEnv(stub)
    for call in (lambda: mixed.compute_done(np.zeros(6), np.zeros(6), {}), lambda: mixed.attach_her(32), lambda: mixed.compute_reward(np.zeros(6), np.zeros(6), {})):
        with pytest.raises(NotImplementedError, match="goal-env relabelling is per task"):
            call()


def test_attach_her_refusals():
    env = _goal_env("ReachHuman", n=2)
    assert env.her is None and env.horizon == 12
    with pytest.raises(NotImplementedError, match="online_sampling"):
        env.attach_her(32, online_sampling=False)
    for size in (5, 12):
        with pytest.raises(ValueError, match="horizon"):
            env.attach_her(size)
    with pytest.raises(NotImplementedError, match="another backend"):   # the oracle backend has no kernels
        env.attach_her(13)
    assert env.her is None
    env.close()
    # collision prevention behind the IK front-end: the executed action is a joint action, the policy's space is Cartesian
    clips = hrg.synthetic_clips(2, seed=0, min_frames=200, max_frames=300)
    kw, fe = dict(shield_type="OFF", horizon=12, seed=6), dict(ik_position_delta=dict(action_limit=0.15), collision_prevention=dict(replace_type=0, n_resamples=20))
    desc = hrg.build_model_desc(kw, n_clips=clips.n_clips, env_id="PickPlaceHumanCart", **fe)
    both = hrg.HipVecEnv(2, env_id="PickPlaceHumanCart", env_kwargs=kw, clips=clips, goal_env=True, backend=OracleBackend(desc, clips, 2), **fe)
    with pytest.raises(NotImplementedError, match="collision prevention behind the IK front-end"):
        both.attach_her(32)
    both.close()
    # either front-end alone: the stored action is rescaled by the policy's action bounds
    for one, width in ((dict(ik_position_delta=fe["ik_position_delta"]), 4), (dict(collision_prevention=fe["collision_prevention"]), 7)):
        desc = hrg.build_model_desc(kw, n_clips=clips.n_clips, env_id="PickPlaceHumanCart", **one)
        env = hrg.HipVecEnv(2, env_id="PickPlaceHumanCart", env_kwargs=kw, clips=clips, goal_env=True, backend=OracleBackend(desc, clips, 2), **one)
        d = env._her_desc(2, 32, 4, "future", False, None)
        assert (d.act_dim, d.rescale_actions) == (width, 1)
        assert list(d.act_high[:width]) == [float(x) for x in env.action_space.high] and list(d.act_low[:width]) == [float(x) for x in env.action_space.low]
        env.close()


def test_abi_names_constants_and_the_header_stays_in_the_base_translation_unit():
    from human_robot_gym_amd import _lib
    from human_robot_gym_amd._cstruct import PROTOTYPES, HerDesc
    import ctypes
    for s in ("hrg_her_create", "hrg_her_destroy", "hrg_her_observe", "hrg_her_add", "hrg_her_sample", "hrg_her_counts", "hrg_her_export", "hrg_goal_reward_done"):
        assert s in _lib.EXPORTS
    vp = ctypes.c_void_p
    assert PROTOTYPES["hrg_her_create"] == (ctypes.c_int, [vp, ctypes.c_int32, vp]) and PROTOTYPES["hrg_her_destroy"] == (None, [vp])
    assert PROTOTYPES["hrg_her_sample"][1] == [vp, ctypes.c_int32] + [vp] * 12
    assert PROTOTYPES["hrg_goal_reward_done"][1] == [vp] * 4 + [ctypes.c_int32] + [vp] * 3
    assert (CONST["HRG_GOAL_REACH"], CONST["HRG_GOAL_CUBE"]) == (0, 1)
    assert (CONST["HRG_HER_FUTURE"], CONST["HRG_HER_FINAL"], CONST["HRG_HER_EPISODE"]) == (0, 1, 2) and CONST["HRG_HER_INDEX_DIM"] == 3
    fields = dict(HerDesc._fields_)
    assert set(fields) == {"n_envs", "capacity", "horizon", "goal_kind", "strategy", "her_ratio", "seed", "goal_dist", "task_reward", "object_gripped_reward",
                           "reward_shaping", "collision_reward", "reward_scale", "done_at_success", "done_at_collision", "act_dim", "act_low", "act_high",
                           "rescale_actions", "n_obs_cols", "obs_cols", "relabel_observation", "n_dg_in_obs", "dg_in_obs"}
    assert fields["obs_cols"]._length_ == 64 and fields["dg_in_obs"]._length_ == 8 and fields["act_low"]._length_ == 7
    base = open(_lib.SRC).read()
    at = base.index('#include "hrgym_her.h"')
    assert base.rindex("#if HRG_BASE_TU", 0, at) > base.rindex("#endif", 0, at)   # inside the block that only the base translation unit compiles
    assert at > base.index('#include "hrgym_dataset.h"')
    for src in _lib.SOURCES[1:]:
        assert "hrgym_her.h" not in open(src).read(), src
    assert len(_lib.SOURCES) == 12
    assert any(d.endswith("hrgym_her.h") for d in _lib.library_dependencies())
    her = open(_lib.SRC.replace("hrgym_hip.hip", "hrgym_her.h")).read()
    assert "STREAM_HER = 10" in her


def test_her_desc_of_an_env_and_the_config_translation():
    from human_robot_gym_amd.her import her_ratio
    from human_robot_gym_amd.training_utils import her_kwargs_from_config
    env = _goal_env("PickPlaceHumanCart", n=2, reward_shaping=True, collision_reward=-3.0)
    d = env._her_desc(2, 40, 4, "final", True, 9)
    assert (d.n_envs, d.capacity, d.horizon, d.goal_kind, d.strategy, d.seed) == (2, 40, 12, CONST["HRG_GOAL_CUBE"], CONST["HRG_HER_FINAL"], 9)
    assert d.her_ratio == her_ratio(4) == 0.8 and (d.goal_dist, d.collision_reward, d.reward_shaping) == (0.6, -3.0, 1)
    assert d.object_gripped_reward == env._desc.object_gripped_reward and d.task_reward == env._desc.task_reward
    assert (d.act_dim, d.rescale_actions) == (7, 0)
    assert d.n_obs_cols == len(env._cols) == 30 and list(d.obs_cols[:30]) == list(env._cols)
    assert d.relabel_observation == 1 and d.n_dg_in_obs == 3 and list(d.dg_in_obs[:3]) == [27, 28, 29]   # object-state 12, robot0_proprio-state 15, desired_goal
    assert [env._cols[k] for k in d.dg_in_obs[:3]] == list(env._dg_cols)
    assert env._her_desc(2, 40, 4, "future", False, None).seed == 6 and env._her_desc(2, 40, 4, "future", False, None).n_dg_in_obs == 0
    with pytest.raises(ValueError, match="goal_selection_strategy"):
        env._her_desc(2, 40, 4, "random", False, None)
    env.close()
    alg = NS(buffer_size=1_000_000, replay_buffer_kwargs=NS(n_sampled_goal=4, goal_selection_strategy="future", online_sampling=True))
    cfg = NS(run=NS(env_type="goal_env", n_envs=4096), algorithm=alg, environment=NS(horizon=100))
    assert her_kwargs_from_config(cfg) == dict(n_sampled_goal=4, goal_selection_strategy="future", online_sampling=True, buffer_size=244)
    cfg.run.n_envs = 100_000   # never less than two episodes per env
    assert her_kwargs_from_config(cfg)["buffer_size"] == 202
    assert her_kwargs_from_config(NS(run=NS(env_type="env", n_envs=4), algorithm=alg, environment=NS(horizon=100))) is None
    assert her_kwargs_from_config(NS(run=NS(env_type="goal_env", n_envs=4), algorithm=NS(buffer_size=10), environment=NS(horizon=100))) is None
    with pytest.raises(NotImplementedError, match="replay_buffer_kwargs"):
        her_kwargs_from_config(NS(run=NS(env_type="goal_env", n_envs=4), algorithm=NS(replay_buffer_kwargs=dict(copy_info_dict=True)), environment=NS(horizon=100)))


# ---- self-checks of her_ref -------------------------------------------------------------------------------------------------------------------------
def _check_ring(ring, written):
    """tail <= open <= w, at most cap stored, tail and open at episode starts, every closed slot carries its episode, counter by counter."""
    for e in range(ring.n):
        w, tail, opn = int(ring.w[e]), int(ring.tail[e]), int(ring.open[e])
        assert 0 <= tail <= opn <= w and w - tail <= ring.cap
        i = tail
        while i < opn:
            s = i % ring.cap
            L = int(ring.ep_len[e, s])
            assert L >= 1 and ring.ep_start[e, s] == i and i + L <= opn
            for k in range(L):
                sk = (i + k) % ring.cap
                assert ring.ep_start[e, sk] == i and ring.ep_len[e, sk] == L
                assert ring.done[e, sk] == (k == L - 1)
                np.testing.assert_array_equal(ring.post[e, sk], written[e][i + k])   # the slot still holds that counter's transition
            i += L
        assert i == opn
        for i in range(opn, w):
            assert ring.ep_len[e, i % ring.cap] == 0 and ring.ep_start[e, i % ring.cap] == opn


def test_her_ref_ring_invariants_under_wrap_and_masked_observe():
    n, cap, horizon = 3, 8, 5
    ring, written = R.Ring(n, cap), [dict() for _ in range(n)]
    ring.observe(np.zeros((n, 64), np.float32))
    dropped = 0
    for k, (a, obs, term, rew, done, info) in enumerate(R.scripted_steps(n, 60, horizon, seed=1)):
        tail0 = ring.tail.copy()
        for e in range(n):
            written[e][int(ring.w[e])] = term[e] if done[e] else obs[e]
        ring.add(a, obs, term, rew, done, info)
        dropped += int((ring.tail > tail0).sum())
        _check_ring(ring, written)
        if k == 30:   # a masked reset in mid-episode discards env 1's open episode only
            assert ring.w[1] > ring.open[1] and ring.w[0] > ring.open[0]
            w0 = ring.w.copy()
            ring.observe(obs + 1, mask=np.array([0, 1, 0], np.uint8))
            assert ring.w[1] == ring.open[1] and ring.w[0] == w0[0] and ring.w[2] == w0[2]
            np.testing.assert_array_equal(ring.cur_obs[1], obs[1] + 1)
            np.testing.assert_array_equal(ring.cur_obs[0], obs[0])
            _check_ring(ring, written)
    assert dropped >= 10 and np.all(ring.w > 5 * cap)   # the ring wrapped several times and whole episodes left it


def test_her_ref_sampler_stays_inside_closed_episodes(oracle_lib):
    u01 = oracle_lib.hrgo_test_u01
    n, cap, horizon = 4, 16, 6
    ring = R.Ring(n, cap)
    ring.observe(np.zeros((n, 64), np.float32))
    steps = list(R.scripted_steps(n, 45, horizon, seed=2))
    for a, obs, term, rew, done, info in steps:
        done[3] = 0   # env 3 never closes an episode ...
        if ring.w[3] - ring.open[3] == horizon - 1:
            ring.observe(obs, mask=np.array([0, 0, 0, 1], np.uint8))   # ... it is reset instead
        ring.add(a, obs, term, rew, done, info)
    assert ring.counts()[3] == 0 and np.all(ring.counts()[:3] > 0) and np.any(ring.w[:3] > ring.open[:3])
    for strategy in ("future", "final", "episode"):
        for ratio in (0.0, 0.8, 1.0):
            s = R.sample(ring, u01, 11, 3, 300, "reach", ratio, strategy)
            e, i = s["index"][:, 0], s["index"][:, 1]
            assert np.all(e != 3) and set(e.tolist()) == {0, 1, 2}
            assert np.all(i >= ring.tail[e]) and np.all(i < ring.open[e])           # never an open or a dropped slot
            assert np.all(ring.ep_start[e, i % cap] + s["t"] == i) and np.all(s["L"] == ring.ep_len[e, i % cap]) and np.all(s["L"] >= 1)
            lo = s["t"] if strategy == "future" else np.zeros_like(s["t"])
            assert np.all(s["f"] >= lo) and np.all(s["f"] < s["L"])
            if strategy == "final":
                assert np.all(s["f"] == s["L"] - 1)
            assert s["relabel"].mean() == ratio if ratio in (0.0, 1.0) else 0.7 < s["relabel"].mean() < 0.9
            rl = s["relabel"]
            np.testing.assert_array_equal(s["index"][rl, 2], (ring.ep_start[e, i % cap] + s["f"])[rl])
            assert np.all(s["index"][~rl, 2] == -1)
            # a sample relabelled with its own outcome is a success of the reach rule; the others keep reward and the done flag without timeouts
            own = rl & (s["f"] == s["t"])
            assert np.all(s["reward"][own, 0] == R.PARAMS["task_reward"])
            keep = ~rl
            np.testing.assert_array_equal(s["reward"][keep, 0], ring.reward[e, i % cap][keep].astype(np.float64))
            np.testing.assert_array_equal(s["done"][keep, 0], (ring.done[e, i % cap] & (1 - ring.truncated[e, i % cap]))[keep])
    a, b = R.sample(ring, u01, 11, 3, 257, "reach", 0.8), R.sample(ring, u01, 11, 3, 65, "reach", 0.8)
    for key in ("index", "observation", "desired_goal", "reward"):
        np.testing.assert_array_equal(a[key][:65], b[key])   # a sample does not depend on the size of its batch
    assert not np.array_equal(R.sample(ring, u01, 11, 4, 65, "reach", 0.8)["index"], b["index"])   # but on the call


def test_her_ref_reward_done_is_the_env_arithmetic():
    """her_ref.reward_done against HipVecEnv.compute_reward / compute_done on random goal rows around the threshold."""
    rng = np.random.RandomState(3)
    for env_id, kind in (("ReachHuman", "reach"), ("PickPlaceHumanCart", "cube")):
        for shaping in (False, True):
            env = _goal_env(env_id, n=2, reward_shaping=shaping, collision_reward=-3.0, reward_scale=2.0, done_at_success=True, done_at_collision=True)
            d = env._desc
            p = {k: getattr(d, k) for k in R.PARAMS}
            ag = rng.uniform(-1, 1, (64, len(R.AG_COLS[kind]))).astype(np.float32)
            if kind == "cube":
                ag[:, 6] = rng.randint(0, 2, 64)
            dg = (ag[:, :6] if kind == "reach" else ag[:, 3:6]) + (rng.uniform(-1, 1, (64, len(R.DG_COLS[kind]))) * rng.choice([0.2, 3.0] if kind == "reach" else [0.1, 1.0], (64, 1))).astype(np.float32)
            ctype = rng.choice([0, 1, 2, 4, 8, 16], 64)
            infos = [dict(collision_type=int(c)) for c in ctype]
            r, dn = R.reward_done(kind, p, ag, dg, ctype)
            np.testing.assert_array_equal(r.astype(np.float32), env.compute_reward(ag, dg, infos))
            np.testing.assert_array_equal(dn, env.compute_done(ag, dg, infos))
            assert 5 < (R.goal_distance(kind, ag, dg) <= p["goal_dist"]).sum() < 59
            env.close()
