"""The task table of the Python package (human_robot_gym_amd/tasks.py): closed over the package, and one value per trait pinned to the reference's own files.
No GPU: the C side's answer to a task id without a row comes before hrg_batch_create touches a device."""
import ctypes

import pytest

import human_robot_gym_amd as hrg
from human_robot_gym_amd import _lib
from human_robot_gym_amd._cstruct import CONST
from human_robot_gym_amd.dataset import SIR_KINDS
from human_robot_gym_amd.expert import EXPERT_ENVS, EXPERT_KWARGS
from human_robot_gym_amd.tasks import TASKS, Goal, task_row, value
from human_robot_gym_amd.vec_env import OBS_COLUMNS, task_columns

TASK_IDS = {v for k, v in CONST.items() if k.startswith("HRG_TASK_")}
SIR_IDS = {CONST[k] for k in ("HRG_SIR_REACH", "HRG_SIR_PICK_PLACE", "HRG_SIR_LIFTING")}   # the kinds with a reward (the other HRG_SIR_* are HRG_SIR_NONE and columns)


def test_the_tasks_are_the_eleven():
    assert set(TASKS) == {"ReachHuman", "ReachHumanCart", "PickPlaceHumanCart", "PickPlaceCloseHumanCart", "PickPlacePointingHumanCart", "HumanObjectInspectionCart",
                          "HumanRobotHandoverCart", "RobotHumanHandoverCart", "CollaborativeLiftingCart", "CollaborativeStackingCart", "CollaborativeHammeringCart"}
    # every HRG_TASK_* has a row; HRG_TASK_REACH_BOX is ReachHuman's with reach_box=True
    assert {t.task for t in TASKS.values()} | {task_row("ReachHuman", reach_box=True).task} == TASK_IDS


@pytest.mark.parametrize("env_id", sorted(TASKS))
def test_a_row_is_closed_over_the_package(env_id):
    t = TASKS[env_id]
    assert t.task in TASK_IDS and (t.sir is None or t.sir in SIR_IDS and t.sir != CONST["HRG_SIR_NONE"])
    assert t.world in ("reach", "pick_place", "hammering") and t.block in (None, "box", "stack", "hammer")
    assert set(t.experts) <= set(EXPERT_KWARGS)
    cols = task_columns(env_id)
    assert all(k in cols and all(0 <= c < CONST["HRG_OBS_DIM"] for c in cols[k]) for k in t.obs_keys), t.obs_keys
    assert all(0 <= c < CONST["HRG_OBS_DIM"] for v in t.columns.values() for c in v)
    if isinstance(t.goal, Goal):   # a goal specification ...
        assert t.goal.rule in ("distance", "cube") and t.goal.achieved and t.goal.desired
        assert (t.goal.kind in ("reach", "cube")) != bool(t.goal.no_kind)   # a device goal kind, or the reason there is none
        assert list(cols["desired_goal"]) == list(t.goal.desired)
    else:                          # ... or the reason the task cannot be a goal env
        assert isinstance(t.goal, str) and t.goal
    assert set(dict(t.info_aliases)) <= {"n_object_handed_over"}   # the one task-specific info column
    assert isinstance(value(t.clip_extra), dict) and set(value(t.clip_env_kwargs)) <= set(t.env_kwargs)
    d = hrg.build_model_desc(env_id=env_id)
    assert d.task == t.task and d.horizon == t.env_kwargs["horizon"]


@pytest.mark.parametrize("env_id,reach_box", [(e, False) for e in sorted(TASKS)] + [("ReachHuman", True)])
def test_the_env_takes_the_experts_its_row_lists_and_no_other(env_id, reach_box):
    """HipVecEnv refuses an expert the row does not list before it builds anything (so: no GPU); one it lists gets as far as the missing GPU."""
    from human_robot_gym_amd.vec_env import HipVecEnv
    import torch
    for eid in EXPERT_KWARGS:
        expert = dict(id=eid, **({"signal_to_noise_ratio": 1.0, "board_size": [1.0, 0.4, 0.03]} if eid == "CollaborativeLiftingCart" else {}))
        if eid not in task_row(env_id, reach_box).experts:
            with pytest.raises(NotImplementedError, match=f"expert {eid}: it reads the observation of"):
                HipVecEnv(2, env_id=env_id, expert=expert, reach_box=reach_box)
        elif not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                HipVecEnv(2, env_id=env_id, expert=expert, reach_box=reach_box, ik_position_delta=None if eid == "ReachHuman" else dict(action_limit=0.1))


def test_reach_box_is_a_switch_of_the_reachhuman_row():
    t, b = TASKS["ReachHuman"], task_row("ReachHuman", reach_box=True)
    assert (t.task, t.block) == (CONST["HRG_TASK_REACH"], None) and (b.task, b.block, b.experts, b.sir) == (CONST["HRG_TASK_REACH_BOX"], "box", (), None)
    assert (b.env_kwargs, b.obs_keys, b.goal) == (t.env_kwargs, t.obs_keys, t.goal)
    assert hrg.build_model_desc(env_id="ReachHuman", reach_box=True).task == CONST["HRG_TASK_REACH_BOX"]
    with pytest.raises(ValueError, match="belongs to ReachHuman"):
        hrg.build_model_desc(env_id="PickPlaceHumanCart", reach_box=True)


def test_one_value_per_trait_as_the_reference_has_it():
    """Expected values written from the reference's files (paths under human_robot_gym/), not from the table."""
    T = TASKS
    # task constant: class PickPlaceCloseHumanCart(PickPlaceHumanCart) (environments/manipulation/pick_place_close_human_cartesian_env.py:19) overrides no step logic
    assert T["PickPlaceCloseHumanCart"].task == T["PickPlaceHumanCart"].task == CONST["HRG_TASK_PICK_PLACE"]
    # default env kwargs: training/config/environment/default/reach_human_cart.yaml (goal_dist: 0.05  # reach_human: 0.1)
    assert T["ReachHumanCart"].env_kwargs["goal_dist"] == 0.05 and T["ReachHuman"].env_kwargs["goal_dist"] == 0.1
    # object block: CollaborativeStackingEnvState(HumanEnvState) (collaborative_stacking_cartesian_env.py:64) carries the cubes' own state; ReachHumanCart(ReachHuman)
    # (reach_human_cartesian_env.py:27) keeps ReachHuman's smallBox
    assert T["CollaborativeStackingCart"].block == "stack" and T["ReachHumanCart"].block == "box"
    # default obs_keys: training/config_icra_2024/environment_evaluation/training/CS-SAC.yaml:177-180 (run.obs_keys begins ...)
    assert T["CollaborativeStackingCart"].obs_keys[:3] == ["object_gripped", "vec_eef_to_all_objects", "gripper_aperture"]
    # column overlay: ReachHumanCart's goal is an end-effector position, three values (reach_human_cartesian_env.py:338-378)
    assert len(task_columns("ReachHumanCart")["goal_difference"]) == 3 and len(task_columns("ReachHuman")["goal_difference"]) == 6
    # info alias: info["max_stack_height"] (collaborative_stacking_cartesian_env.py:677)
    assert dict(T["CollaborativeStackingCart"].info_aliases) == {"n_object_handed_over": "max_stack_height"}
    # experts: expert.id of PP-AIR.yaml:147, CS-AIR.yaml:145, HRH-AIR.yaml:141, RHH-AIR.yaml:142 (config_icra_2024/environment_evaluation/training/) is PickPlaceHumanCart;
    # CL-AIR.yaml:142 CollaborativeLiftingCart, R-AIR.yaml:139 ReachHuman
    assert EXPERT_ENVS["PickPlaceHumanCart"] == ("PickPlaceHumanCart", "CollaborativeStackingCart", "HumanRobotHandoverCart", "RobotHumanHandoverCart")
    assert EXPERT_ENVS["CollaborativeLiftingCart"] == ("CollaborativeLiftingCart",) and EXPERT_ENVS["ReachHuman"] == ("ReachHuman",)
    # state imitation reward: ReachHumanStateBasedExpertImitationRewardWrapper (wrappers/state_based_expert_imitation_reward_wrapper.py:283) reads goal_difference, which
    # ReachHumanCart(ReachHuman) observes too; the pick-place wrapper (416) serves "any environment that can be solved using the PickPlaceHumanCartExpert"
    assert SIR_KINDS["ReachHumanCart"] == SIR_KINDS["ReachHuman"] == CONST["HRG_SIR_REACH"]
    assert SIR_KINDS["RobotHumanHandoverCart"] == CONST["HRG_SIR_PICK_PLACE"] and "HumanObjectInspectionCart" not in SIR_KINDS
    # goals: ReachHuman's are joint angles (reach_human_env.py:477-507): robot0_joint_pos against desired_goal
    g = T["ReachHuman"].goal
    assert (list(g.achieved), list(g.desired), g.rule) == (list(OBS_COLUMNS["robot0_joint_pos"]), list(OBS_COLUMNS["desired_goal"]), "distance")


def test_a_task_id_without_a_row_is_an_unknown_task():
    """hrg_batch_create answers a task id above the last one with "unknown task", before it touches a device."""
    lib = _lib.load_library()
    clips = hrg.synthetic_clips(1, min_frames=10, max_frames=20)
    table, h = clips.table(), ctypes.c_void_p()
    for task in (max(TASK_IDS) + 1, -1):
        desc = hrg.build_model_desc(n_clips=1)
        desc.task = task
        assert lib.hrg_batch_create(ctypes.byref(desc), ctypes.byref(table), 2, 0, 0, ctypes.byref(h)) == CONST["HRG_ERR_UNSUPPORTED"]
        assert lib.hrg_last_error().decode() == "unknown task" and not h.value
