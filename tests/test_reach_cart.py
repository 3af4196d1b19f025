"""ReachHumanCart without a GPU: the numpy restatement tests/reach_cart_ref.py (kinematics, goal sampling, observables, rewards, the scripted expert against
the reference's recorded actions), the task's defaults against the reference's settings files, the translation of its configs, the model description."""
import math
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest

import human_robot_gym_amd as hrg
import reach_cart_ref as R
from human_robot_gym_amd import _lib, dataset as D, model as M
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.expert import EXPERT_ENVS, build_expert_desc, expert_kwargs
from test_assets import REF, _compose, _same

ENV = "ReachHumanCart"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reach_cart_ref.npz")
CFG = os.path.join(REF, "training", "config")
INIT = [0.0, 0.0, -math.pi / 2, 0.0, -math.pi / 2, math.pi / 4]
NARM = CONST["HRG_NARM"]


def _desc(**kw):
    return hrg.build_model_desc(dict(seed=5, **kw), env_id=ENV)


def test_model_description():
    d = _desc()
    assert d.task == CONST["HRG_TASK_REACH_CART"] == 10 and d.goal_dist == 0.05
    assert list(d.init_qpos) == INIT
    assert [list(d.sampling_space[0]), list(d.sampling_space[1])] == [[0.1, -0.5, 0.8], [0.5, 0.5, 1.3]]
    box = hrg.build_model_desc(dict(seed=5), env_id="ReachHuman", reach_box=True)   # the same world: the smallBox, the table, the obstacle margin
    for f in ("box_half", "box_inertia", "obj_bin", "tgt_bin", "table_half"):
        assert list(getattr(d, f)) == list(getattr(box, f)), f
    assert (d.box_mass, d.obj_z, d.obstacle_margin, d.n_goals, d.horizon) == (box.box_mass, box.obj_z, box.obstacle_margin, box.n_goals, box.horizon)
    assert box.task == CONST["HRG_TASK_REACH_BOX"] and list(box.init_qpos) == [0.0] * NARM
    e = _desc(init_joint_pos=[0.1] * NARM, sampling_space=[[1, 1, 1], [0, 0, 0]])
    assert list(e.init_qpos) == [0.1] * NARM and list(e.sampling_space[0]) == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="reach_box"):
        hrg.build_model_desc(None, env_id=ENV, reach_box=True)
    with pytest.raises(NotImplementedError, match="table_friction"):
        _desc(table_friction=[1.5, 2.0, 0.05])
    with pytest.raises(ValueError, match="sampling_space"):
        _desc(sampling_space=[0.1, 0.5])
    with pytest.raises(NotImplementedError, match="sampling_space"):   # a keyword of this task alone
        hrg.build_model_desc(dict(sampling_space=[[0, 0, 0], [1, 1, 1]]), env_id="ReachHuman")
    assert len(_lib.SOURCES) == 12   # the task adds no translation unit


def test_defaults_are_the_reference_settings_files():
    """ENV_DEFAULTS / EXPERT_KWARGS / the state imitation reward's arguments against training/config/{environment, expert, wrappers/state_based_...}/ with their
    defaults lists composed; init_joint_pos and sampling_space are the constructor's (reach_human_cartesian_env.py:280-283: not in any settings file)."""
    ref = _compose(os.path.join(CFG, "environment", "reach_human_cart.yaml"))
    mine = M.ENV_DEFAULTS[ENV]
    ref["table_friction"] = [float(x) for x in ref["table_friction"]]     # (yaml.safe_load reads 5e-3, written without a dot, as a string)
    assert ref["env_id"] == ENV and ref["goal_dist"] == 0.05 and ref["table_friction"] == [1.0, 5e-3, 1e-4]
    common = [k for k in mine if k in ref]
    assert len(common) >= 20 and {"goal_dist", "table_friction", "horizon", "done_at_success"} <= set(common)
    bad = {k: (mine[k], ref[k]) for k in common if not _same(mine[k], ref[k])}
    assert not bad, bad
    assert "init_joint_pos" not in ref and "sampling_space" not in ref and _same(mine["init_joint_pos"], INIT)
    # ... and apart from those keywords (the table's size is the one compiled into ReachHuman's arena: a keyword here so that the task's config passes) the task is ReachHuman
    assert _same(mine["table_full_size"], ref["table_full_size"])
    assert {k for k in mine if k not in M.ENV_DEFAULTS["ReachHuman"] or not _same(mine[k], M.ENV_DEFAULTS["ReachHuman"][k])} == {"goal_dist", "table_friction", "table_full_size", "init_joint_pos", "sampling_space"}
    ex = _compose(os.path.join(CFG, "expert", "reach_human_cart.yaml"))
    assert ex["id"] == ENV and ex["obs_keys"] == ["goal_difference"] and ex["signal_to_noise_ratio"] == 0.95
    eid, kw = expert_kwargs(ex)
    assert eid == ENV and kw == dict(signal_to_noise_ratio=0.95, delta_time=0.01, seed=None)
    own = _compose(os.path.join(CFG, "expert", "default", "reach_human_cart.yaml"))
    assert expert_kwargs(dict(id=ENV))[1] == {k: own[k] for k in ("signal_to_noise_ratio", "delta_time", "seed")}
    assert EXPERT_ENVS[ENV] == (ENV,)
    sb = _compose(os.path.join(CFG, "wrappers", "state_based_expert_imitation_reward", "reach_human_cart_state_based_expert_imitation_reward.yaml"))
    assert (sb["iota"], sb["sim_fn"], sb["et_dist"], sb["alpha"], sb["observe_time"], sb["use_et"]) == (0.1, "gaussian", 2, 0, True, False)
    p = D.sir_kwargs(ENV, sb)
    assert p == dict(alpha=0.0, observe_time=True, use_et=False, et_dist=2.0, beta=1.0, iota_m=0.1, iota_g=1.0, m_sim_fn="gaussian", g_sim_fn="gaussian")
    assert D.SIR_KINDS[ENV] == CONST["HRG_SIR_REACH"]


def _data_collection_config():
    """training/config/reach_human_cart_expert_data_collection.yaml with its groups composed by hand: environment reach_human_cart, wrappers safe_ik
    (collision prevention + the IK front-end at their default files), expert reach_human_cart, then the file's own overrides."""
    import yaml
    top = yaml.safe_load(open(os.path.join(CFG, "reach_human_cart_expert_data_collection.yaml")))
    assert {"environment": "reach_human_cart"} in top["defaults"] and {"expert": "reach_human_cart"} in top["defaults"] and {"wrappers": "safe_ik"} in top["defaults"]
    env = dict(_compose(os.path.join(CFG, "environment", "reach_human_cart.yaml")), **top["environment"])
    ex = dict(_compose(os.path.join(CFG, "expert", "reach_human_cart.yaml")), **top["expert"])
    assert ex["seed"] == "${run.seed}"
    ex["seed"] = 7   # the interpolation, resolved
    wr = dict(collision_prevention=yaml.safe_load(open(os.path.join(CFG, "wrappers", "collision_prevention", "default_collision_prevention.yaml"))),
              ik_position_delta=yaml.safe_load(open(os.path.join(CFG, "wrappers", "ik_position_delta", "default_ik_position_delta.yaml"))))
    return NS(environment=env, expert=ex, wrappers=wr, robot=NS(name="Schunk"), run=NS(seed=7, obs_keys=top["run"]["obs_keys"]), dataset_name=top["dataset_name"], n_episodes=top["n_episodes"])


def test_configs_translate(tmp_path, monkeypatch):
    cfg = _data_collection_config()
    kw = hrg.wrapper_kwargs_from_config(cfg)
    assert set(kw) == {"collision_prevention", "ik_position_delta"} and float(kw["ik_position_delta"]["action_limit"]) == 0.15
    from human_robot_gym_amd.training_utils import compose_environment_kwargs
    ekw = compose_environment_kwargs(cfg)
    assert ekw["done_at_success"] is False and ekw["goal_dist"] == 0.05 and "env_id" not in ekw
    d = hrg.build_model_desc(ekw, env_id=cfg.environment["env_id"], **kw)
    assert d.task == CONST["HRG_TASK_REACH_CART"] and d.ik_enabled == 1 and d.cp_enabled == 1 and d.done_at_success == 0
    eid, ek = expert_kwargs(cfg.expert)
    assert (eid, ek) == (ENV, dict(signal_to_noise_ratio=0.98, delta_time=0.01, seed=7))
    x = build_expert_desc(cfg.expert, [-0.15] * 3 + [-1], [0.15] * 3 + [1])
    assert (x.expert, x.cartesian, x.seed, x.signal_to_noise_ratio, x.act_high[0]) == (CONST["HRG_EXPERT_REACH_CART"], 1, 7, 0.98, 0.15)
    # the action-based imitation reward with this expert: only on its own environment
    ab = NS(dataset_name="reach-cart-dataset", alpha=0.25, rsi_prob=None, beta=1.0, iota_m=0.1, iota_g=0.25, m_sim_fn="gaussian", g_sim_fn="gaussian")
    cfg.wrappers["action_based_expert_imitation_reward"] = ab
    kw = hrg.wrapper_kwargs_from_config(cfg)
    assert kw["expert"] == dict(id=ENV, signal_to_noise_ratio=0.98, seed=7, delta_time=0.01) and kw["imitation_reward"]["alpha"] == 0.25
    pp = NS(environment=dict(env_id="PickPlaceHumanCart"), expert=cfg.expert, wrappers=dict(action_based_expert_imitation_reward=ab))
    with pytest.raises(NotImplementedError, match=ENV):
        hrg.wrapper_kwargs_from_config(pp)
    # the state-based imitation reward config, once a dataset of that name exists below the working directory
    sb = _compose(os.path.join(CFG, "wrappers", "state_based_expert_imitation_reward", "reach_human_cart_state_based_expert_imitation_reward.yaml"))
    assert sb["dataset_name"] == "${run.dataset_name}"
    sb["dataset_name"] = "reach-cart-dataset"
    del cfg.wrappers["action_based_expert_imitation_reward"]
    cfg.wrappers["state_based_expert_imitation_reward"] = sb
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match="hrg_dataset.npz"):
        hrg.wrapper_kwargs_from_config(cfg)
    os.makedirs(tmp_path / "datasets" / "reach-cart-dataset")
    (tmp_path / "datasets" / "reach-cart-dataset" / "hrg_dataset.npz").write_bytes(b"")
    kw = hrg.wrapper_kwargs_from_config(cfg)
    assert kw["dataset"] == "reach-cart-dataset" and kw["rsi_prob"] == 0.0
    assert D.sir_kwargs(ENV, kw["state_imitation_reward"])["iota_m"] == 0.1


def test_eef_position_and_velocity():
    d = _desc()
    Rk, pk = M.robot_fk_numpy(d, INIT + [0.0, 0.0])                     # the host's table-building kinematics: another walk over the same description
    np.testing.assert_allclose(R.eef_pos(d, INIT), pk[NARM - 1] + Rk[NARM - 1] @ np.array(list(d.eef_pos)), rtol=0, atol=1e-14)
    assert R.in_space(d, R.eef_pos(d, INIT))                            # the initial posture holds the gripper inside the sampling space
    rng = np.random.RandomState(0)
    for _ in range(5):   # eef_velp is the time derivative of eef_pos along qvel: central difference, error O(h^2 |q'''|) ~ 1e-8 at h = 1e-4
        q, v, h = rng.uniform(-1.5, 1.5, NARM), rng.uniform(-1, 1, NARM), 1e-4
        fd = (R.eef_pos(d, q + h * v) - R.eef_pos(d, q - h * v)) / (2 * h)
        np.testing.assert_allclose(R.eef_velp(d, q, v), fd, rtol=0, atol=1e-6)
    assert np.all(R.eef_velp(d, INIT, np.zeros(NARM)) == 0)


def test_goal_sampling(oracle_lib):
    u01 = oracle_lib.hrgo_test_u01
    d = _desc()
    lo, hi = np.array(list(d.qpos_limits[0])[:NARM]), np.array(list(d.qpos_limits[1])[:NARM])
    accepted, fallback = 0, 0
    for gid in range(40):
        q, e = R.candidates(d, u01, gid, 1, 2)
        assert np.all(q >= lo) and np.all(q <= hi)
        assert q[3, 4] == lo[4] + (hi[4] - lo[4]) * u01(5, gid, 1, R.STREAM_GOAL, (2 * 20 + 3) * NARM + 4)        # the kernels' draw keys
        inside = [R.in_space(d, x) for x in e]
        goal, tgt, t, _ = R.sample_goal(d, u01, gid, 1, 2)
        if any(inside):
            assert t == inside.index(True) and np.array_equal(goal, q[t]) and np.array_equal(tgt, e[t]) and R.in_space(d, tgt)
            accepted += 1
            # a collision check that refuses the accepted candidate moves the goal to a later one, or to the fallback
            g2, t2_tgt, t2, _ = R.sample_goal(d, u01, gid, 1, 2, collides=lambda x, bad=q[t]: np.array_equal(x, bad))
            later = [k for k in range(t + 1, 20) if inside[k]]
            assert t2 == (later[0] if later else -1)
        else:
            assert t == -1 and list(goal) == INIT and np.array_equal(tgt, R.eef_pos(d, INIT))     # the fallback is the initial posture, not zeros
            fallback += 1
    assert accepted >= 5 and fallback >= 1, (accepted, fallback)
    empty = _desc(sampling_space=[[1, 1, 1], [0, 0, 0]])
    goal, tgt, t, _ = R.sample_goal(empty, u01, 0, 1, 0)
    assert t == -1 and list(goal) == INIT
    assert R.face_margin(d, np.array([0.3, 0.0, 0.8 + 1e-10])) == pytest.approx(1e-10, rel=1e-3)


def test_distance_success_and_rewards():
    d, ds = _desc(task_reward=2.0, collision_reward=-5.0, reward_scale=0.5), _desc(reward_shaping=True)
    tgt = np.array([0.3, 0.1, 1.0])
    eef = np.array([[0.3, 0.1, 1.0], [0.3, 0.1, 1.05], [0.3, 0.1, 1.0500001], [0.6, 0.5, 1.0]])
    dist = R.distance(eef, tgt)
    np.testing.assert_allclose(dist, [0.0, 0.05, 0.0500001, 0.5], rtol=0, atol=1e-15)
    ok = R.success(d, dist)
    assert list(ok) == [True, dist[1] <= 0.05, False, False] and not R.success(d, 0.0, crash=True)
    np.testing.assert_allclose(R.reward(d, dist, ok, illegal=np.array([False, False, True, False])), np.where(ok, 1.0, -0.5) + np.array([0, 0, -2.5, 0]))
    np.testing.assert_allclose(R.reward(ds, dist, R.success(ds, dist)), np.where(ok, 1.0, -1.0) + 1.0 - 0.1 * dist)
    np.testing.assert_array_equal(R.goal_difference(tgt, eef[3]), tgt - eef[3])


def test_expert_restatement_reproduces_the_reference_actions():
    with np.load(GOLDEN) as z:
        fx = {k: z[k] for k in z.files}
    gd, want = fx["cart_goal_difference"], fx["cart_action"]
    assert gd.shape == (321, 3) and want.shape == (321, 4) and np.all(gd.astype(np.float32) == gd)
    lim = fx["cart_high"][0]
    assert np.abs(np.abs(gd) - lim).min() >= 1e-9 and (np.abs(gd) > lim).any() and np.all(want[:, 3] == 0)
    np.testing.assert_array_equal(R.expert(gd, fx["cart_low"], fx["cart_high"]), want)      # clip alone at signal_to_noise_ratio 1: exact
    nz = np.full((321, 3), 0.05)
    half = R.expert(gd, fx["cart_low"], fx["cart_high"], 0.5, nz)
    np.testing.assert_allclose(half[:, :3], np.clip(0.5 * want[:, :3] + 0.025, -lim, lim), rtol=0, atol=1e-16)


def test_columns_and_refusals_without_a_batch():
    from human_robot_gym_amd.vec_env import DEFAULT_OBS_KEYS, OBS_COLUMNS_TASK, task_columns
    cols = task_columns(ENV)
    assert list(cols["goal_difference"]) == [12, 13, 14] and list(cols["desired_goal"]) == [33, 34, 35] and list(cols["robot0_eef_velp"]) == [40, 41, 42]
    assert list(cols["robot0_eef_pos"]) == [30, 31, 32] and list(cols["object-state"]) == list(range(12))
    assert "robot0_eef_velp" in OBS_COLUMNS_TASK[ENV] and DEFAULT_OBS_KEYS[ENV] == ["object-state", "goal_difference"]
    assert list(task_columns("ReachHuman")["goal_difference"]) == list(range(12, 18))         # ReachHuman keeps its six
    with pytest.raises(NotImplementedError, match="ReachHumanCart"):                          # the expert reads this task's observation only
        hrg.HipVecEnv(2, env_id="ReachHuman", expert=dict(id=ENV))
    for other in ("ReachHuman", "PickPlaceHumanCart"):                                        # columns 40:43 hold other quantities elsewhere: the key is this task's
        with pytest.raises(NotImplementedError, match="robot0_eef_velp"):
            hrg.HipVecEnv(2, env_id=other, obs_keys=["object-state", "robot0_eef_velp"])
