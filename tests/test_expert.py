"""Scripted experts + action-based imitation reward, host side (no GPU): tests/expert_ref.py (the restatement the GPU tests compare the kernels
with) against the recorded outputs of the reference's own expert classes (tests/golden/expert_ref.npz, tools/make_expert_fixtures.py), and the
translation of `config.expert` / `config.wrappers.action_based_expert_imitation_reward` into HipVecEnv keyword arguments."""
import ast
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest

import human_robot_gym_amd as hrg
import expert_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expert_ref.npz")
ROWS = 321   # one full 256-thread block of the expert kernel + 65
# add, clip, sqrt and one division at magnitude <= 1 on f32-representable inputs: both sides round each operation to half an ulp (1.1e-16 at 1)
ATOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    d["pp_params"], d["cl_params"] = ast.literal_eval(str(d["pp_params"])), ast.literal_eval(str(d["cl_params"]))
    return d


def test_fixture_inputs_are_f32_and_cover_every_branch(fx):
    for k in ("reach_goal_difference", "pp_vec_eef_to_object", "pp_vec_eef_to_target", "pp_robot0_gripper_qpos", "cl_vec_eef_to_human_lh", "cl_vec_eef_to_human_rh",
              "hm_vec_eef_to_nail"):
        assert fx[k].shape[0] == ROWS and fx[k].dtype == np.float64
        np.testing.assert_array_equal(fx[k], fx[k].astype(np.float32).astype(np.float64))
    assert np.bincount(fx["pp_motion_branch"], minlength=5).min() >= 20 and fx["pp_motion_branch"].max() == 4
    assert np.bincount(fx["pp_gripper_branch"], minlength=3).min() >= 20 and fx["pp_gripper_branch"].max() == 2
    assert float(fx["pp_dropped_share"]) <= 0.01
    pp = {k: v for k, v in fx["pp_params"].items() if k != "delta_time"}
    pred, margin = R.pick_place_predicates(fx["pp_object_gripped"], fx["pp_vec_eef_to_object"], fx["pp_vec_eef_to_target"], fx["pp_robot0_gripper_qpos"], **pp)
    assert margin.min() >= 1e-9
    mb, gb = R.pick_place_branches(pred, pp["release_when_delivered"])   # the restatement takes the branches the reference's own predicates took
    np.testing.assert_array_equal(mb, fx["pp_motion_branch"])
    np.testing.assert_array_equal(gb, fx["pp_gripper_branch"])
    assert "stand-ins" in str(fx["note"])


def test_restatement_reproduces_every_recorded_expert_action(fx):
    pp = {k: v for k, v in fx["pp_params"].items() if k != "delta_time"}
    cl = {k: v for k, v in fx["cl_params"].items() if k != "delta_time"}
    lim, glim = fx["cart_high"][0], fx["cart_high"][3]
    got = dict(
        reach=R.reach(fx["reach_goal_difference"], fx["joint_low"], fx["joint_high"]),
        pp=R.pick_place(fx["pp_object_gripped"], fx["pp_vec_eef_to_object"], fx["pp_vec_eef_to_target"], fx["pp_robot0_gripper_qpos"], lim, glim, **pp),
        cl=R.lifting(fx["cl_vec_eef_to_human_lh"], fx["cl_vec_eef_to_human_rh"], lim, glim, **cl),
        hm=R.hammering(fx["hm_vec_eef_to_nail"]),
    )
    for k, a in got.items():
        want = fx[k + "_action"]
        assert a.shape == want.shape == (ROWS, 7 if k == "reach" else 4)
        np.testing.assert_allclose(a, want, rtol=0, atol=ATOL, err_msg=k)
    # the same through the observation superset's columns (what the kernel reads)
    full = np.zeros((ROWS, 64))
    full[:, 39] = fx["pp_object_gripped"]
    full[:, 40:43], full[:, 43:46], full[:, 53:55] = fx["pp_vec_eef_to_object"], fx["pp_vec_eef_to_target"], fx["pp_robot0_gripper_qpos"]
    np.testing.assert_allclose(R.expert_from_obs("PickPlaceHumanCart", full, fx["cart_low"], fx["cart_high"], **pp), fx["pp_action"], rtol=0, atol=ATOL)


def test_restatement_reproduces_the_similarity_grid(fx):
    for name in ("gaussian", "tanh"):
        got = R.similarity(name, fx["sim_delta"][:, None], fx["sim_iota"][None, :])
        np.testing.assert_allclose(got, fx["sim_" + name], rtol=1e-15, atol=0)
    assert R.similarity("gaussian", 0.1, 0.1) == 0.5   # iota is the half width at half maximum (the tanh form gives 0.5023 there)
    with pytest.raises(ValueError):
        R.similarity("cosine", 0.1, 0.1)


def test_reward_mix_and_noise_recursion():
    a = np.array([[0.05, 0.0, -0.02, 1.0]])
    x = np.array([[0.05, 0.0, 0.08, -1.0]])
    r_im, r_m, r_g = R.imitation_reward(a, x, beta=0.7, iota_m=0.1, iota_g=0.5)
    assert r_m[0] == pytest.approx(0.5) and r_g[0] == pytest.approx(2.0 ** -16) and r_im[0] == pytest.approx(0.7 * 0.5 + 0.3 * 2.0 ** -16)
    assert R.combine(r_im, np.array([-1.0]), 0.25)[0] == pytest.approx(0.25 * r_im[0] - 0.75)
    assert R.combine(r_im, np.array([-1.0]), 0.0)[0] == -1.0
    j = np.zeros((1, 7)); j[0, 0] = 0.5
    _, r_m, _ = R.imitation_reward(j, np.zeros((1, 7)), 1.0, 0.5, 0.5, normalize_joint_actions=True, low=-2 * np.ones(7), high=2 * np.ones(7))
    assert r_m[0] == pytest.approx(2.0 ** -0.25)   # normalised distance 0.25
    # the recursion's own fixed point: var' = (1 - alpha dt)^2 var + b^2
    al, sg, dt = 10.0, 0.5, 0.01
    v = R.ou_stationary_variance(al, sg, dt)
    assert (1 - al * dt) ** 2 * v + (sg * np.sqrt(2 * al) * np.sqrt(dt)) ** 2 == pytest.approx(v, rel=1e-14)
    assert R.ou_step(np.array([1.0]), np.array([0.0]), al, sg, dt)[0] == pytest.approx(0.9)


def _pp_air_config(rsi_prob=None, expert_id="PickPlaceHumanCart", with_expert=True):
    """The shape of config_icra_2024/environment_evaluation/training/PP-AIR.yaml's wrappers / expert nodes."""
    cfg = NS(
        wrappers=NS(collision_prevention=NS(replace_type=0, n_resamples=20),
                    ik_position_delta=NS(urdf_file="models/assets/robots/schunk/robot_pybullet.urdf", action_limit=0.1, x_output_max=1, x_position_limits=None,
                                         residual_threshold=0.001, max_iter=50),
                    action_based_expert_imitation_reward=NS(dataset_name="pick-place-dataset", alpha=0.25, rsi_prob=rsi_prob, beta=0.7, iota_m=0.1, iota_g=0.5,
                                                            m_sim_fn="gaussian", g_sim_fn="gaussian")))
    if with_expert:
        cfg.expert = NS(id=expert_id, signal_to_noise_ratio=0.98, hover_dist=0.2, tan_theta=0.5, horizontal_epsilon=0.035, vertical_epsilon=0.015, goal_dist=0.08,
                        gripper_fully_opened_threshold=0.02, release_when_delivered=True, delta_time=0.01, seed=5,
                        obs_keys=["object_gripped", "vec_eef_to_object", "vec_eef_to_target", "robot0_gripper_qpos"])
    return cfg


def test_wrapper_kwargs_of_a_pp_air_config_without_reference_state_initialisation():
    kw = hrg.wrapper_kwargs_from_config(_pp_air_config(rsi_prob=None))
    assert kw["imitation_reward"] == dict(alpha=0.25, beta=0.7, iota_m=0.1, iota_g=0.5, m_sim_fn="gaussian", g_sim_fn="gaussian")
    assert kw["expert"] == dict(id="PickPlaceHumanCart", signal_to_noise_ratio=0.98, hover_dist=0.2, tan_theta=0.5, horizontal_epsilon=0.035, vertical_epsilon=0.015,
                                goal_dist=0.08, gripper_fully_opened_threshold=0.02, release_when_delivered=True, delta_time=0.01, seed=5)
    assert kw["collision_prevention"] == dict(replace_type=0, n_resamples=20) and kw["ik_position_delta"]["action_limit"] == 0.1
    # ... and from there into the kernel argument
    from human_robot_gym_amd.expert import build_expert_desc
    d = build_expert_desc(kw["expert"], [-0.1, -0.1, -0.1, -1], [0.1, 0.1, 0.1, 1], kw["imitation_reward"])
    assert (d.expert, d.cartesian, d.reward_enabled, d.seed, d.m_sim_fn, d.release_when_delivered) == (1, 1, 1, 5, 0, 1)
    assert (d.horizontal_epsilon, d.signal_to_noise_ratio, d.alpha, d.beta, d.iota_g, d.act_high[0], d.act_low[3]) == (0.035, 0.98, 0.25, 0.7, 0.5, 0.1, -1.0)


def test_unsupported_imitation_configs_fail_loudly():
    with pytest.raises(NotImplementedError, match="DatasetRSIWrapper"):
        hrg.wrapper_kwargs_from_config(_pp_air_config(rsi_prob=0.5))
    with pytest.raises(NotImplementedError, match="expert"):
        hrg.wrapper_kwargs_from_config(_pp_air_config(rsi_prob=None, with_expert=False))
    with pytest.raises(NotImplementedError, match="ReachHumanCart"):
        hrg.wrapper_kwargs_from_config(_pp_air_config(rsi_prob=None, expert_id="ReachHumanCart"))
    # unchanged: alpha = 0 without an expert node (rsi_prob null or 0) leaves the environment reward as it is and is skipped
    for rsi in (None, 0.0):
        cfg = _pp_air_config(rsi_prob=rsi, with_expert=False)
        cfg.wrappers.action_based_expert_imitation_reward.alpha = 0.0
        kw = hrg.wrapper_kwargs_from_config(cfg)
        assert "expert" not in kw and "imitation_reward" not in kw
    from human_robot_gym_amd.expert import build_expert_desc
    with pytest.raises(TypeError, match="normalize_joint_actions"):   # the Cart wrapper has no such argument
        build_expert_desc(dict(id="PickPlaceHumanCart"), [-0.1] * 3 + [-1], [0.1] * 3 + [1], dict(alpha=0.25, normalize_joint_actions=False))
    assert build_expert_desc(dict(id="ReachHuman"), [-1] * 7, [1] * 7, dict(alpha=0.25, normalize_joint_actions=True)).normalize_joint_actions == 1
    with pytest.raises(TypeError, match="board_size"):
        build_expert_desc(dict(id="CollaborativeLiftingCart", signal_to_noise_ratio=1), [-0.1] * 3 + [-1], [0.1] * 3 + [1])
    with pytest.raises(TypeError, match="hover"):
        build_expert_desc(dict(id="ReachHuman", hover_dist=0.2), [-1] * 7, [1] * 7)


def test_vec_env_refuses_an_expert_it_cannot_run():
    from helpers import OracleBackend
    ex = dict(id="PickPlaceHumanCart")
    with pytest.raises(NotImplementedError, match="backend"):
        hrg.HipVecEnv(2, env_id="PickPlaceHumanCart", backend=OracleBackend, expert=ex, ik_position_delta=dict(action_limit=0.1))
    with pytest.raises(NotImplementedError, match="goal_env"):
        hrg.HipVecEnv(2, env_id="PickPlaceHumanCart", goal_env=True, expert=ex, ik_position_delta=dict(action_limit=0.1))
    with pytest.raises(NotImplementedError, match="observation"):
        hrg.HipVecEnv(2, env_id="ReachHuman", expert=ex)
    with pytest.raises(ValueError, match="expert"):
        hrg.HipVecEnv(2, env_id="ReachHuman", imitation_reward=dict(alpha=0.25))
    for kw in (dict(expert=ex), dict(imitation_reward=dict(alpha=0.25))):   # the mixed batch (refused before anything is built)
        with pytest.raises(NotImplementedError, match="per task"):
            hrg.make_mixed_vec_env(4, tasks=[("ReachHuman", {}), ("PickPlaceHumanCart", {})], **kw)


def test_abi_names_the_three_entry_points_and_the_header_is_a_build_dependency():
    from human_robot_gym_amd import _lib
    from human_robot_gym_amd._cstruct import CONST, ExpertDesc
    for s in ("hrg_batch_expert_attach", "hrg_batch_expert_actions", "hrg_batch_step_imitation"):
        assert s in _lib.EXPORTS
    assert CONST["HRG_IMIT_DIM"] == 8 and CONST["HRG_EXPERT_HAMMERING"] == 3 and CONST["HRG_SIM_TANH"] == 1
    assert {"expert", "cartesian", "act_low", "act_high", "signal_to_noise_ratio", "delta_time", "seed", "alpha", "beta", "iota_m", "iota_g", "m_sim_fn", "g_sim_fn",
            "normalize_joint_actions", "reward_enabled", "board_size", "human_grip_offset"} <= {f for f, _ in ExpertDesc._fields_}
    assert os.path.exists(os.path.join(os.path.dirname(_lib.SRC), "hrgym_expert.h"))
