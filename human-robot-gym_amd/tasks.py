"""Every task of the package, once: what an `env_id` is, beyond the model `build_model_desc` fills for it.

One frozen `Task` row per `env_id` in `TASKS`; the C host side keeps the counterpart per `HRG_TASK_*` (csrc/hrgym_host_batch.h: HRG_TASKS), and
tests/test_tasks_gpu.py holds the two against each other.  A new task of an existing kernel family is a row here, a row there, its `*_ENV_KWARGS` below and
whatever is new in the kernel and the descriptor.  Nothing of the package is imported here but the constants of include/hrgym.h.
"""
import math
from dataclasses import dataclass, replace
from typing import Any, Optional, Tuple, Union

from ._cstruct import CONST

# default kwargs = HumanEnv/ReachHuman constructor defaults overlaid with config/environment/reach_human.yaml
DEFAULT_ENV_KWARGS = dict(
    robots="Schunk", robot_base_offset=[0.0, 0.0, 0.0], reward_scale=1.0, reward_shaping=False, collision_reward=0, task_reward=1,
    done_at_collision=False, done_at_success=True, control_freq=10, horizon=100, shield_type="SSM", control_sample_time=0.004,
    base_human_pos_offset=[0.0, 0.0, 0.0], human_animation_freq=120, human_rand=[0.0, 0.0, 0.0], n_animations_sampled_per_100_steps=5,
    n_goals_sampled_per_100_steps=20, goal_dist=0.1, safe_vel=0.01, self_collision_safety=0.012, collision_debounce_delay=0.01, seed=0,
)

# ReachHumanCart: config/environment/reach_human_cart.yaml, which composes default/reach_human_cart.yaml (goal_dist, table_friction) over default/reach_human.yaml
# and repeats reach_human.yaml's own keys.  init_joint_pos is the constructor's default (reach_human_cartesian_env.py:280); sampling_space is an attribute the
# reference's constructor sets (283) -- a keyword here: [lower corner, upper corner] of the box a goal's end-effector position has to lie in
REACH_CART_ENV_KWARGS = dict(
    DEFAULT_ENV_KWARGS,
    goal_dist=0.05,
    table_full_size=[1.5, 2.0, 0.05],     # default/reach_human.yaml: the arena compiled into the asset tables; accepted at this value only, like table_friction
    table_friction=[1.0, 5e-3, 1e-4],
    init_joint_pos=[0.0, 0.0, -math.pi / 2, 0.0, -math.pi / 2, math.pi / 4],
    sampling_space=[[0.1, -0.5, 0.8], [0.5, 0.5, 1.3]],
)
# PickPlaceHumanCart constructor defaults overlaid with config/environment/pick_place_human_cart.yaml (+ default/human_env.yaml)
PICK_PLACE_ENV_KWARGS = dict(
    DEFAULT_ENV_KWARGS, horizon=1000, done_at_success=False, safe_vel=0.001, self_collision_safety=0.01, table_full_size=[1.5, 2.0, 0.05],
    object_full_size=[0.04, 0.04, 0.04], n_object_placements_sampled_per_100_steps=3, n_targets_sampled_per_100_steps=3, object_gripped_reward=-0.25,
)
# HumanObjectInspectionCart constructor defaults overlaid with config/environment/(default/)human_object_inspection_cart.yaml
INSPECTION_ENV_KWARGS = dict(
    PICK_PLACE_ENV_KWARGS, human_rand=[0.0, 0.5, 0.0], n_animations_sampled_per_100_steps=2,
    n_targets_sampled_per_100_steps=0,      # the target comes with the animation (human_object_inspection_cartesian_env.py:394)
    object_gripped_reward=-1.0, object_at_target_reward=-1.0, goal_exit_tolerance=0.02,
)
# PickPlaceCloseHumanCart: PickPlaceHumanCart with clips recorded at 60 Hz (pick_place_close_human_cartesian_env.py:219-285)
PICK_PLACE_CLOSE_ENV_KWARGS = dict(PICK_PLACE_ENV_KWARGS, human_animation_freq=60, object_gripped_reward=-1.0)
# PickPlacePointingHumanCart + config/environment/pick_place_pointing_human_cart.yaml
POINTING_ENV_KWARGS = dict(PICK_PLACE_ENV_KWARGS, horizon=500, object_gripped_reward=-1.0)
# HumanRobotHandoverCart constructor defaults overlaid with config/environment/(default/)human_robot_handover_cart.yaml
HANDOVER_H2R_ENV_KWARGS = dict(
    PICK_PLACE_ENV_KWARGS, shield_type="PFL", table_full_size=[1.0, 2.0, 0.05], human_animation_freq=90, human_rand=[0.0, 0.2, 0.1],
    n_animations_sampled_per_100_steps=2, n_targets_sampled_per_100_steps=3, object_at_target_reward=0.0, object_gripped_reward=-0.25,
    collision_reward=-1.0, goal_exit_tolerance=0.0, done_at_success=True,
)
# RobotHumanHandoverCart constructor defaults overlaid with config/environment/(default/)robot_human_handover_cart.yaml
HANDOVER_R2H_ENV_KWARGS = dict(
    PICK_PLACE_ENV_KWARGS, shield_type="PFL",
    table_full_size=[1.5, 2.0, 0.05],   # (round 3: was the human-to-robot task's 1.0 m table by mistake; robot_human_handover_cartesian_env.py:305, RHH-*.yaml:63-66)
    human_animation_freq=90, human_rand=[0.0, 0.2, 0.1], n_animations_sampled_per_100_steps=2, n_targets_sampled_per_100_steps=0, goal_dist=0.06,
    object_in_human_hand_reward=0.0, object_gripped_reward=-0.25, collision_reward=-1.0, done_at_success=True,
)
# CollaborativeLiftingCart constructor defaults (collaborative_lifting_cartesian_env.py:215-280) overlaid with
# config/environment/(default/)collaborative_lifting_cart.yaml
LIFTING_ENV_KWARGS = dict(
    PICK_PLACE_ENV_KWARGS, horizon=5000, table_full_size=[0.4, 1.5, 0.05], board_full_size=[1.0, 0.4, 0.03],
    board_density=20.0,                 # BoxObject(name="board", density=20), 755-760
    board_released_reward=-10.0, imbalance_failure_reward=-10.0, min_balance=0.8, collision_reward=0, reward_shaping=True, done_at_success=True,
    human_animation_freq=20, human_rand=[0.0, 0.0, 0.0], n_animations_sampled_per_100_steps=0.2, safe_vel=0.001,
    lift_anchors=[[-0.45, 0.25, 0.0], [-0.45, -0.25, 0.0]],   # l_anchor / r_anchor of _postprocess_model, 786-795
)
# CollaborativeStackingCart constructor defaults (collaborative_stacking_cartesian_env.py:316-386) overlaid with
# config/environment/(default/)collaborative_stacking_cart.yaml
STACKING_ENV_KWARGS = dict(
    PICK_PLACE_ENV_KWARGS, horizon=3000, table_full_size=[1.2, 2.0, 0.05], object_full_size=[0.045, 0.045, 0.045], goal_dist=0.025,
    n_object_placements_sampled_per_100_steps=2, n_animations_sampled_per_100_steps=5, collision_reward=0.0, stack_toppled_reward=-10.0,
    task_reward=2.0, second_cube_at_target_reward=0.0, fourth_cube_at_target_reward=1.0, object_gripped_reward=0.75, human_rand=[0.02, 0.1, 0.1],
    done_at_success=True,
    stack_weld_relpos=[0.0, 0.045, 0.0],   # relpose of lh_weld_eq / rh_weld_eq (1263-1281)
)
# CollaborativeHammeringCart constructor defaults (collaborative_hammering_cartesian_env.py:291-367) overlaid with training/config/environment/default/
# collaborative_hammering_cart.yaml (table / board sizes, sampling rates) and, on top, the TOP-LEVEL training/config/environment/collaborative_hammering_cart.yaml
# -- the convention of every other task here (what make_vec_env(env_id) steps is what the reference's training config for that env would step).  The top-level
# file sets collision_reward 0, nail_hammered_in_reward 0.0, done_at_success false; its defaults list composes default/pick_place_human_cart instead of
# default/collaborative_hammering_cart (a quirk of the reference: the task has no experiment config), which is NOT followed -- the task's own default file is.
HAMMERING_ENV_KWARGS = dict(
    PICK_PLACE_ENV_KWARGS,
    horizon=1000,
    table_full_size=[1.5, 2.0, 0.05],
    board_full_size=[1.0, 0.4, 0.03],
    n_nail_placements_sampled_per_100_steps=1,
    goal_tolerance=0.05,
    collision_reward=0.0,
    hammer_gripped_reward_bonus=0.0,
    nail_hammered_in_reward=0.0,
    done_at_collision=False,
    done_at_success=False,
    task_reward=1.0,
    human_animation_freq=100,
    human_rand=[0.0, 0.0, 0.0],
    n_animations_sampled_per_100_steps=5,   # default/human_env.yaml:60 through the task's default file (the constructor's own default is 1; round 3: was 1)
    gripper_controllable=False,
    noslip_iterations=20,       # self.sim.model.opt.noslip_iterations = 20 (_setup_references, 1161); 0 switches the pass off (round 2's model: the nail creeps)
    noslip_tolerance=1e-6,      # MuJoCo's default opt.noslip_tolerance
    nail_frictionloss=10000.0,  # nail.xml:7 (10 000 N = model.NAIL["frictionloss"]); a model parameter so that tests can show a nail yielding to a force above it
    hammer_anchors=[[-0.1, 0.2, 0.0], [-0.5, -0.2, 0.0]],   # l_anchor / r_anchor of _postprocess_model (1001-1002)
    hammer_weld_relquat=[0.0, 0.0, 0.0, 1.0],               # relpose of rh_eq: "0 0 0 0 0 0 1" (1123-1131)
)

OBS_KEYS = ["object-state", "goal_difference"]  # default: training/config/human_reach_ppo_parallel.yaml:14-16
# training/config/run/obs_keys of the pick-place experiments (e.g. PP-SAC): the observables the policy sees; the inspection, pointing and handover tasks take them too
PICK_PLACE_OBS_KEYS = ["object_gripped", "vec_eef_to_object", "vec_eef_to_target", "gripper_aperture", "dist_eef_to_human_head",
                       "dist_eef_to_human_lh", "dist_eef_to_human_rh"]
STACKING_OBS_KEYS = ["object_gripped", "vec_eef_to_all_objects", "gripper_aperture", "dist_eef_to_human_head", "dist_eef_to_human_lh", "dist_eef_to_human_rh"]   # CS-SAC.yaml run.obs_keys
LIFTING_OBS_KEYS = ["board_quat", "dist_eef_to_human_head", "vec_eef_to_human_lh", "vec_eef_to_human_rh"]   # CL-SAC.yaml run.obs_keys
HAMMERING_OBS_KEYS = ["hammer_gripped", "vec_eef_to_nail", "nail_hammering_progress", "vec_eef_to_board", "board_quat", "dist_eef_to_human_head", "dist_eef_to_human_lh",
                      "dist_eef_to_human_rh"]   # no run config ships for this task; the expert reads vec_eef_to_nail (collaborative_hammering_cart_expert.py:24-25)


@dataclass(frozen=True)
class Goal:
    """A task as a goal env (GoalEnvironmentGymWrapper, wrappers/goal_env_wrapper.py): the columns of the observation superset that are its goals, and the
    rule of `compute_reward` / `compute_done`: "distance" = the Euclidean distance of the two goals, "cube" = the cube tasks' rule over
    [eef_pos, object_pos, object_gripped] vs target_pos (pick_place_human_cartesian_env.py:528-611)."""
    achieved: Tuple[int, ...]
    desired: Tuple[int, ...]
    rule: str
    kind: Optional[str] = None      # goal kind of the device buffers and the device feature row (HRG_GOAL_*: "reach" | "cube"); None: there is none, and ...
    no_kind: Optional[str] = None   # ... this is the reason `attach_her` gives


@dataclass(frozen=True)
class Task:
    task: int                        # HRG_TASK_*
    env_kwargs: dict                 # the default environment keyword arguments (ENV_DEFAULTS)
    world: str                       # the block of build_model_desc that fills its descriptor fields: "reach" | "pick_place" | "hammering"
    block: Optional[str]             # the per-env object block next to hrg_env_state: None | "box" | "stack" | "hammer"
    obs_keys: list                   # the default obs_keys
    columns: dict                    # where its observables sit when not where vec_env.OBS_COLUMNS has them (`task_columns`)
    goal: Union[Goal, str]           # its goal specification, or the reason it cannot be a goal env
    experts: Tuple[str, ...] = ()    # the expert ids (expert.EXPERT_KWARGS) that read its observation
    sir: Optional[int] = None        # HRG_SIR_* of its StateBasedExpertImitationRewardWrapper subclass (state_based_expert_imitation_reward_wrapper.py); None: it has none
    info_aliases: Any = ()           # {info key: the name this task gives the column}
    clip_extra: Any = ()             # keywords of animation.synthetic_clips that make the clips carry the animation info it reads (a dict, or a callable returning one) ...
    clip_env_kwargs: Any = ()        # ... and the env kwargs that go with those clips (the reference's defaults belong to its recorded clips)


def _hammering_clips():
    from .animation import HAMMERING_HANDS
    return dict(hammering=HAMMERING_HANDS)


def _hammering_clip_env_kwargs():
    from .animation import hammering_relquat
    return dict(hammer_weld_relquat=hammering_relquat())


def _lifting_clips():
    from .animation import lifting_hands_nominal
    from .model import build_model_desc
    return dict(lifting=lifting_hands_nominal(build_model_desc(None, env_id="CollaborativeLiftingCart")), fps=20.0)


_PHASE = "this task's success is a task phase, not a function of the goals"
_TARGET = {"desired_goal": range(50, 53)}   # _get_desired_goal_from_obs of the cube tasks: target_pos
# the cube tasks' goals: [robot0_eef_pos, object_pos, object_gripped] vs target_pos (pick_place_human_cartesian_env.py:574-611)
_CUBE_GOAL = Goal(achieved=(30, 31, 32, 47, 48, 49, 39), desired=(50, 51, 52), rule="cube", kind="cube")

TASKS = {
    # ReachHuman: joint-angle goals (reach_human_env.py:477-507).  The lean model without the task's smallBox; `task_row(..., reach_box=True)` is the one with it
    "ReachHuman": Task(CONST["HRG_TASK_REACH"], DEFAULT_ENV_KWARGS, "reach", None, OBS_KEYS, {},
                       Goal(achieved=tuple(range(18, 24)), desired=tuple(range(33, 39)), rule="distance", kind="reach"),
                       experts=("ReachHuman",), sir=CONST["HRG_SIR_REACH"]),
    # ReachHumanCart (reach_human_cartesian_env.py:385-434): the ReachHuman layout, the goal an end-effector position (three values; the other three columns are
    # zero); achieved goal = robot0_eef_pos, desired goal = the goal's eef position (338-378).  The Reach state reward reads its three goal_difference columns
    "ReachHumanCart": Task(CONST["HRG_TASK_REACH_CART"], REACH_CART_ENV_KWARGS, "reach", "box", OBS_KEYS,
                           {"goal_difference": range(12, 15), "desired_goal": range(33, 36), "robot0_eef_velp": range(40, 43), "goal-state": list(range(33, 36)) + list(range(12, 15))},
                           Goal(achieved=(30, 31, 32), desired=(33, 34, 35), rule="distance",
                                no_kind="achieved = robot0_eef_pos, desired = the goal's eef position: HRG_GOAL_REACH relabels joint angles, HRG_GOAL_CUBE object positions"),
                           experts=("ReachHumanCart",), sir=CONST["HRG_SIR_REACH"]),
    "PickPlaceHumanCart": Task(CONST["HRG_TASK_PICK_PLACE"], PICK_PLACE_ENV_KWARGS, "pick_place", "box", PICK_PLACE_OBS_KEYS, _TARGET, _CUBE_GOAL,
                               experts=("PickPlaceHumanCart",), sir=CONST["HRG_SIR_PICK_PLACE"]),
    "PickPlaceCloseHumanCart": Task(CONST["HRG_TASK_PICK_PLACE"], PICK_PLACE_CLOSE_ENV_KWARGS, "pick_place", "box", PICK_PLACE_OBS_KEYS, _TARGET, _CUBE_GOAL),
    "PickPlacePointingHumanCart": Task(CONST["HRG_TASK_POINTING"], POINTING_ENV_KWARGS, "pick_place", "box", PICK_PLACE_OBS_KEYS, _TARGET, _CUBE_GOAL),
    "HumanObjectInspectionCart": Task(CONST["HRG_TASK_INSPECTION"], INSPECTION_ENV_KWARGS, "pick_place", "box", PICK_PLACE_OBS_KEYS, _TARGET, _PHASE,
                                      clip_extra=dict(inspection=True)),
    # CS-AIR runs the pick-place expert; the four cubes + stack bookkeeping are CollaborativeStackingEnvState (collaborative_stacking_cartesian_env.py:63-97)
    "CollaborativeStackingCart": Task(CONST["HRG_TASK_STACKING"], STACKING_ENV_KWARGS, "pick_place", "stack", STACKING_OBS_KEYS, _TARGET, _PHASE,
                                      experts=("PickPlaceHumanCart",), info_aliases={"n_object_handed_over": "max_stack_height"},   # include/hrgym.h HRG_INFO_MAX_STACK_HEIGHT
                                      clip_extra=dict(stacking=True)),
    # HRH-AIR, RHH-AIR run the pick-place expert; the pick-place state reward serves "any environment that can be solved using the PickPlaceHumanCartExpert"
    "HumanRobotHandoverCart": Task(CONST["HRG_TASK_HANDOVER_H2R"], HANDOVER_H2R_ENV_KWARGS, "pick_place", "box", PICK_PLACE_OBS_KEYS, _TARGET, _CUBE_GOAL,
                                   experts=("PickPlaceHumanCart",), sir=CONST["HRG_SIR_PICK_PLACE"], clip_extra=dict(handover=True)),
    "RobotHumanHandoverCart": Task(CONST["HRG_TASK_HANDOVER_R2H"], HANDOVER_R2H_ENV_KWARGS, "pick_place", "box", PICK_PLACE_OBS_KEYS, _TARGET, _CUBE_GOAL,
                                   experts=("PickPlaceHumanCart",), sir=CONST["HRG_SIR_PICK_PLACE"], clip_extra=dict(handover="r2h")),
    "CollaborativeLiftingCart": Task(CONST["HRG_TASK_LIFTING"], LIFTING_ENV_KWARGS, "pick_place", "box", LIFTING_OBS_KEYS, _TARGET, _PHASE,
                                     experts=("CollaborativeLiftingCart",), sir=CONST["HRG_SIR_LIFTING"], clip_extra=_lifting_clips),
    # board, hammer, nail + bookkeeping are CollaborativeHammeringEnvState (collaborative_hammering_cartesian_env.py:56-89)
    "CollaborativeHammeringCart": Task(CONST["HRG_TASK_HAMMERING"], HAMMERING_ENV_KWARGS, "hammering", "hammer", HAMMERING_OBS_KEYS, {
        # collaborative_hammering_cartesian_env.py:1151-1323: the same observable name sits in other columns of the superset (oracle: compute_obs_hammer)
        "hammer_quat": range(12, 16), "board_pos": range(33, 36), "vec_eef_to_board": range(36, 39), "hammer_gripped": range(39, 40),
        "vec_eef_to_hammer": range(40, 43), "vec_eef_to_nail": range(43, 46), "hammer_pos": range(47, 50), "nail_pos": range(50, 53),
        "board_quat": range(57, 61), "nail_hammering_progress": range(61, 62),
        # "object_quat" is never in this env's observation cache, so the two relative quaternions are constant zeros in the reference (1217-1225, 1259-1267)
        "quat_eef_to_hammer": [62, 63, 62, 63], "quat_eef_to_board": [62, 63, 62, 63],
        "desired_goal": range(50, 53),   # _get_desired_goal_from_obs: nail_pos (606-621)
    }, _PHASE, experts=("CollaborativeHammeringCart",), clip_extra=_hammering_clips, clip_env_kwargs=_hammering_clip_env_kwargs),
}


def task_row(env_id, reach_box=False):
    """The row of `env_id`.  `reach_box=True`, a keyword of ReachHuman: the task with its free smallBox object (reach_human_env.py:573-579), stepped by the
    cube kernel.  It carries the box block, and no expert and no state imitation reward fit it: the cube kernel serves object_quat in the goal_difference
    columns."""
    t = TASKS[env_id]
    return replace(t, task=CONST["HRG_TASK_REACH_BOX"], block="box", experts=(), sir=None) if reach_box else t


def value(x):
    """A row's `clip_extra` / `clip_env_kwargs` as a dict: the value itself, or what the callable computes."""
    return dict(x() if callable(x) else x)
