"""Host-side model builder: env kwargs (+ the compiled asset tables) -> hrg_model_desc.

Mirrors what `robosuite.make("ReachHuman", **env_kwargs)` + `FailsafeController.__init__` assemble in the
reference (human_env.py:269-451, reach_human_env.py:226-377, failsafe_controller.py:113-191,
training_utils.py:48-88), but produces one plain-C parameter block for the HIP stepper.

Everything that the reference takes from packages absent from its checkout is a documented SYNTHETIC default
here: the RethinkGripper/RethinkMount geometry [robosuite 1.3.2], MuJoCo solver
defaults, and the three sara-shield YAML files (robot/trajectory/mocap parameters).
"""
import json
import ctypes
import math
import os

import numpy as np

from ._cstruct import CONST, ModelDesc
from .tasks import DEFAULT_ENV_KWARGS, HAMMERING_ENV_KWARGS, TASKS, task_row  # noqa: F401  (a task's default kwargs are its data: tasks.py)

_ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")
ENV_DEFAULTS = {env_id: t.env_kwargs for env_id, t in TASKS.items()}   # what make_vec_env(env_id) steps: the reference's training config for that env

# models/robots/config/schunk.json (qpos_limits) — the only key of that file the controller reads
SCHUNK_QPOS_LIMITS = [[-2.9, -1.8, -2.60, -2.9, -1.85, -2.9], [2.9, 1.8, 2.60, 2.9, 1.85, 2.9]]
# controllers/failsafe_controller/config/failsafe.json
FAILSAFE_CONFIG = dict(input_max=1, input_min=-1, output_max=0.2, output_min=-0.2, kp=100, damping_ratio=1)

# models/objects/human/human.py:57-81 — order of the 23 measured joints handed to the shield
HUMAN_JOINT_ELEMENTS = [
    "L_Hip", "R_Hip", "Torso", "L_Knee", "R_Knee", "Spine", "L_Ankle", "R_Ankle", "Chest", "L_Toe", "R_Toe",
    "Neck", "L_Thorax", "R_Thorax", "Head", "L_Shoulder", "R_Shoulder", "L_Elbow", "R_Elbow", "L_Wrist",
    "R_Wrist", "L_Hand", "R_Hand",
]

# Stand-in for robosuite 1.3.2's composite HammerObject (absent; its dimensions are drawn at random per instance): a box handle at the middle of the
# reference's ranges (handle_radius 0.015-0.02, handle_length 0.1-0.25, handle_density 100-250) and ONE box for head + neck + face
# (head_halfsize between 1 and 1.2 handle radii, head_density_ratio 2); no claw.  Body frame: origin = middle of the handle, handle along z, head along x.
HAMMER = dict(handle_half=[0.0175, 0.0175, 0.0875], handle_density=175.0, head_half=[0.0616, 0.01925, 0.01925], head_density=350.0)
# models/assets/objects/nail.xml: nail_head body 0.06 above nail_base, collision cylinder r 0.02 / half height 0.002 at +0.001 (stand-in: a box of the same
# extents), slide joint along -z, range [0, 0.06], frictionloss 10000, solreffriction (-100, -100)
NAIL = dict(head_half=[0.02, 0.02, 0.002], head_dz=0.001, stem=0.06, range=0.06, frictionloss=10000.0, fric_damping=100.0, dummy_half=0.01)
# RethinkValidGripper.qpos_range (models/grippers/rethink_valid_gripper.py:29-42)
FINGER_QPOS_RANGE = [[-0.0118366, 0.011499], [0.0118366, -0.011499]]

# Synthetic shield parameters (stand-ins for sara-shield's trajectory_parameters_schunk.yaml,
# robot_parameters_schunk.yaml, mujoco_mocap.yaml, which are absent from the reference checkout).
SHIELD_DEFAULTS = dict(
    v_max_allowed=1.0, a_max_allowed=10.0, j_max_allowed=400.0,
    v_max_ltt=1.0, a_max_ltt=2.0, j_max_ltt=15.0,
    secure_radius=0.02,
    ltt_time_sync=True,   # sara-shield's planner synchronises the joints of a long-term trajectory to the slowest one; False: each joint time-optimal (rounds 1-2)
    pfl_v_safe=0.25,   # PFL: Cartesian speed [m/s] the arm may keep when the reachable sets intersect (ISO/TS 15066-style transient contact)
    meas_err_pos=0.0, meas_err_vel=0.0, delay=0.0,
)
# body parts: (proximal joint, distal joint, thickness [m], v_max [m/s], a_max [m/s^2], kept in POS model)
BODY_PARTS = [
    ("L_Hip", "L_Knee", 0.13, 1.6, 20.0, 0), ("R_Hip", "R_Knee", 0.13, 1.6, 20.0, 0),
    ("L_Knee", "L_Ankle", 0.10, 1.6, 20.0, 0), ("R_Knee", "R_Ankle", 0.10, 1.6, 20.0, 0),
    ("L_Ankle", "L_Toe", 0.08, 1.6, 20.0, 0), ("R_Ankle", "R_Toe", 0.08, 1.6, 20.0, 0),
    ("L_Hip", "R_Hip", 0.18, 1.6, 20.0, 1), ("Torso", "Chest", 0.20, 1.6, 20.0, 1),
    ("Chest", "Neck", 0.18, 1.6, 20.0, 1), ("Neck", "Head", 0.15, 1.6, 20.0, 1),
    ("L_Thorax", "L_Shoulder", 0.10, 1.6, 20.0, 1), ("R_Thorax", "R_Shoulder", 0.10, 1.6, 20.0, 1),
    ("L_Shoulder", "L_Elbow", 0.10, 2.0, 50.0, 0), ("R_Shoulder", "R_Elbow", 0.10, 2.0, 50.0, 0),
    ("L_Elbow", "L_Wrist", 0.08, 2.0, 50.0, 0), ("R_Elbow", "R_Wrist", 0.08, 2.0, 50.0, 0),
    ("L_Wrist", "L_Hand", 0.10, 2.0, 50.0, 0), ("R_Wrist", "R_Hand", 0.10, 2.0, 50.0, 0),
]
# extremities of the POS model: (proximal joint, chain of joints to the tip, thickness, v_max of the proximal joint)
EXTREMITIES = [
    ("L_Shoulder", ["L_Elbow", "L_Wrist", "L_Hand"], 0.10, 1.6),
    ("R_Shoulder", ["R_Elbow", "R_Wrist", "R_Hand"], 0.10, 1.6),
    ("L_Hip", ["L_Knee", "L_Ankle", "L_Toe"], 0.13, 1.6),
    ("R_Hip", ["R_Knee", "R_Ankle", "R_Toe"], 0.13, 1.6),
]

# Synthetic RethinkGripper / mount stand-in (robosuite 1.3.2 MJCF is not in the reference tree)
GRIPPER = dict(
    base_z=0.912,                      # height of the robot root on the RethinkMount pedestal
    hand_mass=0.3, hand_inertia=[3e-4, 3e-4, 3e-4],
    finger_mass=0.03, finger_inertia=[0.02, 0.02, 0.02],
    finger_pos=[[0.0, 0.01, 0.0444], [0.0, -0.01, 0.0444]],
    finger_axis=[0.0, 1.0, 0.0],
    finger_range=[[-0.0115, 0.020833], [-0.020833, 0.0115]],
    finger_damping=100.0, finger_armature=1.0, finger_frictionloss=1.0,
    finger_kp=1000.0, finger_forcerange=[-20.0, 20.0],
    finger_init_qpos=[0.0118366, -0.011499],   # RethinkValidGripper.qpos_range[1], rethink_valid_gripper.py:37-42
    speed=0.01,
    grip_site=[0.0, 0.0, 0.109],
    base_capsule=([0.0, 0.0, 0.0], [0.0, 0.0, 0.06], 0.045),
    # pad-side bar of a finger: offset outwards from the finger origin so that the open gripper (qpos_range[1]) spans 6.5 cm
    # and the closed one 1.9 cm between the inner surfaces, parallel to the closing axis normal
    finger_capsule=([0.0, 0.019, 0.03], [0.0, 0.019, 0.09], 0.008),
    shield_capsule=([0.0, 0.0, 0.0], [0.0, 0.0, 0.11], 0.07),
)


def _quat2mat(q):
    w, x, y, z = q
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
    ])


def _merge_inertia(parts):
    """Merge rigid parts [(mass, com(3), I_com(3x3))] expressed in one frame -> (mass, com, I about com)."""
    m = sum(p[0] for p in parts)
    c = sum(p[0] * np.asarray(p[1]) for p in parts) / m
    I = np.zeros((3, 3))
    for mass, com, Ic in parts:
        d = np.asarray(com) - c
        I += np.asarray(Ic) + mass * (d @ d * np.eye(3) - np.outer(d, d))
    return m, c, I


def _seg_seg_dist(p1, q1, p2, q2):
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f = d1 @ d1, d2 @ d2, d2 @ r
    if a <= 1e-12 and e <= 1e-12:
        s = t = 0.0
    elif a <= 1e-12:
        s, t = 0.0, min(1.0, max(0.0, f / e))
    else:
        c = d1 @ r
        if e <= 1e-12:
            t, s = 0.0, min(1.0, max(0.0, -c / a))
        else:
            b = d1 @ d2
            den = a * e - b * b
            s = min(1.0, max(0.0, (b * f - c * e) / den)) if den > 1e-12 * a * e else 0.0
            t = (b * s + f) / e
            if t < 0:
                t, s = 0.0, min(1.0, max(0.0, -c / a))
            elif t > 1:
                t, s = 1.0, min(1.0, max(0.0, (b - c) / a))
    return float(np.linalg.norm((p1 + s * d1) - (p2 + t * d2)))


def _same_list(a, b):
    return len(a) == len(b) and all(float(x) == float(y) for x, y in zip(a, b))


def load_assets(name="reach_human_schunk.json"):
    with open(os.path.join(_ASSETS, name)) as f:
        return json.load(f)


# config/wrappers/ik_position_delta/default_ik_position_delta.yaml (+ the DLS damping, which pybullet keeps internal)
IK_DEFAULTS = dict(action_limit=0.15, x_output_max=1, x_position_limits=None, residual_threshold=1e-3, max_iter=50, damping=0.1)
IK_EE_OFFSET = [0.0, 0.0, 0.17]   # models/assets/robots/schunk/robot_pybullet.urdf:226-228 (fixed_gripper_joint)


# Reference constructor keys that have no effect on the state the stepper computes (rendering, cameras, robosuite plumbing): accepted silently
_NO_EFFECT_KEYS = frozenset((
    "use_camera_obs", "use_object_obs", "has_renderer", "has_offscreen_renderer", "render_camera", "render_collision_mesh", "render_visual_mesh",
    "render_gpu_device_id", "camera_names", "camera_heights", "camera_widths", "camera_depths", "camera_segmentations", "renderer", "renderer_config",
    "visualize_failsafe_controller", "visualize_pinocchio", "verbose", "hard_reset", "ignore_done", "controller_configs"))
# Reference constructor keys that DO change the episode but are not implemented: accepted only at the value listed (the reference's default), else raise
_DEFAULT_ONLY_KEYS = dict(
    env_configuration="default", gripper_types="default", initialization_noise="default", table_friction=[1.0, 5e-3, 1e-4],
    randomize_initial_pos=False, init_joint_pos=None, object_placement_initializer=None, target_placement_initializer=None,
    obstacle_placement_initializer=None)


def _check_env_kwargs(env_id, known, given):
    """Refuse environment keyword arguments that would change the reference's behaviour but are not implemented here, instead of ignoring them
    (`human_animation_names` is the exception: clips are handed over as a ClipSet, the names only select files of the absent animation package)."""
    for k, v in given.items():
        if k in known or k in _NO_EFFECT_KEYS or k == "human_animation_names":
            continue
        if k in _DEFAULT_ONLY_KEYS:
            want = _DEFAULT_ONLY_KEYS[k]
            same = (list(v) == list(want)) if isinstance(want, list) and isinstance(v, (list, tuple)) else (v == want)
            if not same:
                raise NotImplementedError(f"{env_id}: env kwarg {k}={v!r} is not implemented by the HIP stepper (only the reference default {want!r})")
            continue
        raise NotImplementedError(f"{env_id}: unknown env kwarg {k!r} (known: {sorted(known)})")


def load_robot_hulls():
    """(verts [N, 3] float64 C-contiguous, offsets [8] int32): convex hulls of the seven arm collision meshes, compiled by tools/compile_model.py."""
    with np.load(os.path.join(_ASSETS, "schunk_hulls.npz")) as z:
        return np.ascontiguousarray(z["verts"], np.float64), np.ascontiguousarray(z["offsets"], np.int32)


def build_model_desc(env_kwargs=None, n_clips=1, shield_params=None, assets=None, collision_prevention=None, goal_check=True,
                     env_id="ReachHuman", ik_position_delta=None, reach_box=False, robot_geometry="capsule"):
    """Return a filled `ModelDesc` for `env_id` (a key of ENV_DEFAULTS) on the Schunk arm.

    `env_kwargs` takes the same keys as the reference's environment config
    (training/config/environment/reach_human.yaml, default/human_env.yaml).
    `collision_prevention` takes the keys of config/wrappers/collision_prevention/*.yaml (replace_type, n_resamples);
    None = wrapper not in the stack.  `goal_check=False` takes the non-pinocchio branch of `_sample_valid_pos`.
    `reach_box=True` (ReachHuman only) adds the task's free `smallBox` object (reach_human_env.py:573-579) and steps the task with the cube kernel; the default
    is the lean model without it (the box is not observed and only matters when the arm happens to hit it).
    `ik_position_delta` takes the keys of config/wrappers/ik_position_delta/*.yaml (action_limit, x_output_max,
    x_position_limits, residual_threshold, max_iter): actions become [dx, dy, dz, gripper]; None = joint-space actions.
    `robot_geometry`: "capsule" = every arm link collides as the bounding capsule of its mesh; "hull" = as the convex hull of its mesh
    (what MuJoCo makes of a mesh geom) against the human's capsules and the table / floor planes, the capsule being the broadphase.  "hull" covers every task:
    a pair of an arm link with a manipulated object (the cube, the lifting board, a stacking cube, the hammering board, hammer and nail head) is the hull's
    penetration of that box by MPR, one contact per pair; the finger and gripper capsules stay capsules."""
    if env_id not in ENV_DEFAULTS:
        raise NotImplementedError(f"env_id {env_id!r}: the HIP stepper covers {sorted(ENV_DEFAULTS)}")
    task = task_row(env_id, reach_box)
    kw = dict(task.env_kwargs)
    _check_env_kwargs(env_id, kw, env_kwargs or {})
    kw.update(env_kwargs or {})
    sp = dict(SHIELD_DEFAULTS)
    sp.update(shield_params or {})
    A = assets or load_assets()
    robots = kw["robots"]
    if isinstance(robots, (list, tuple)):
        robots = robots[0]
    if robots != "Schunk":
        raise NotImplementedError(f"robot {robots!r}: only the Schunk LWA-4P tables are compiled")
    NV, NARM = CONST["HRG_NV"], CONST["HRG_NARM"]
    d = ModelDesc()
    chain = A["robot"]["chain"]  # link0, link1..link6, right_hand
    off = np.asarray(kw["robot_base_offset"], float)
    d.base_pos[:] = (off + np.array([0.0, 0.0, GRIPPER["base_z"]])).tolist()
    d.base_quat[:] = [1.0, 0.0, 0.0, 0.0]
    links = chain[1:7]
    hand = chain[7]
    R_hand = _quat2mat(np.asarray(hand["quat"]) / np.linalg.norm(hand["quat"]))
    p_hand = np.asarray(hand["pos"])
    for i, L in enumerate(links):
        d.body_pos[i][:] = L["pos"]
        q = np.asarray(L["quat"], float)
        d.body_quat[i][:] = (q / np.linalg.norm(q)).tolist()
        d.body_parent[i] = i - 1
        d.jnt_type[i] = 0
        d.jnt_axis[i][:] = L["axis"]
        d.jnt_range[i][:] = L["range"]
        d.jnt_damping[i] = L["damping"]           # schunk_robot.py:42-45 re-sets the same 1e-4
        d.jnt_frictionloss[i] = L["frictionloss"]
        d.jnt_armature[i] = L["armature"]
        parts = [(L["mass"], L["ipos"], np.diag(L["diaginertia"]))]
        if i == NARM - 1:  # right_hand body + gripper base are welded to link6
            parts.append((hand["mass"], p_hand, np.diag(hand["diaginertia"])))
            parts.append((GRIPPER["hand_mass"], p_hand + R_hand @ np.array([0, 0, 0.03]), np.diag(GRIPPER["hand_inertia"])))
        m, c, I = _merge_inertia(parts)
        d.body_mass[i] = m
        d.body_com[i][:] = c.tolist()
        d.body_inertia[i][:] = [I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]
    # quaternion of the hand frame for the finger bodies
    qh = np.asarray(hand["quat"], float)
    qh = qh / np.linalg.norm(qh)
    for f in range(2):
        i = NARM + f
        d.body_pos[i][:] = (p_hand + R_hand @ np.asarray(GRIPPER["finger_pos"][f])).tolist()
        d.body_quat[i][:] = qh.tolist()
        d.body_parent[i] = NARM - 1
        d.jnt_type[i] = 1
        d.jnt_axis[i][:] = GRIPPER["finger_axis"]
        d.jnt_range[i][:] = GRIPPER["finger_range"][f]
        d.jnt_damping[i] = GRIPPER["finger_damping"]
        d.jnt_frictionloss[i] = GRIPPER["finger_frictionloss"]
        d.jnt_armature[i] = GRIPPER["finger_armature"]
        d.body_mass[i] = GRIPPER["finger_mass"]
        d.body_com[i][:] = [0.0, 0.0, 0.03]
        d.body_inertia[i][:] = GRIPPER["finger_inertia"] + [0.0, 0.0, 0.0]
        d.finger_ctrlrange[f][:] = GRIPPER["finger_range"][f]
        d.finger_init_qpos[f] = GRIPPER["finger_init_qpos"][f]
    d.gravity[:] = [0.0, 0.0, -9.81]
    d.eef_pos[:] = (p_hand + R_hand @ np.asarray(GRIPPER["grip_site"])).tolist()
    for i in range(NARM):
        d.arm_ctrlrange[i][:] = A["robot"]["ctrlrange"][i]
    d.finger_kp = GRIPPER["finger_kp"]
    d.finger_forcerange[:] = GRIPPER["finger_forcerange"]
    d.gripper_speed = GRIPPER["speed"]
    # solver: MuJoCo 2.1 defaults (solref 0.02 1, solimp .9 .95 .001 .5 2, Newton 100 iters tol 1e-8)
    d.timestep = float(kw["control_sample_time"])
    d.solref[:] = [0.02, 1.0]
    d.solimp[:] = [0.9, 0.95, 0.001, 0.5, 2.0]
    d.contact_margin_human = A["human"]["margin"]
    d.friction_static = 1.0
    d.solver_iters = 30
    d.solver_tol = 1e-10
    # ---- collision capsules
    caps = [(-1, chain[0]["capsules"][0])]
    for i, L in enumerate(links):
        caps.append((i, L["capsules"][0]))
    bc = GRIPPER["base_capsule"]
    caps.append((NARM - 1, dict(p1=(p_hand + R_hand @ np.asarray(bc[0])).tolist(), p2=(p_hand + R_hand @ np.asarray(bc[1])).tolist(), r=bc[2])))
    fc = GRIPPER["finger_capsule"]
    caps.append((NARM, dict(p1=fc[0], p2=fc[1], r=fc[2])))
    caps.append((NARM + 1, dict(p1=[fc[0][0], -fc[0][1], fc[0][2]], p2=[fc[1][0], -fc[1][1], fc[1][2]], r=fc[2])))
    assert len(caps) == CONST["HRG_NRCAP"]
    for c, (b, cap) in enumerate(caps):
        d.rcap_body[c] = b
        d.rcap_p1[c][:] = cap["p1"]
        d.rcap_p2[c][:] = cap["p2"]
        d.rcap_r[c] = cap["r"]
    d.table_top_z = A["arena"]["table_top_z"]
    d.table_half[:] = A["arena"]["table_half"]
    d.floor_z = A["arena"]["floor_z"]
    # self-collision candidates: not same body / parent-child, not colliding in the home pose
    # (the rule the reference applies to its pinocchio model: pinocchio_manipulator_model.py:238-270)
    R, p = robot_fk_numpy(d, np.concatenate([np.zeros(NARM), GRIPPER["finger_init_qpos"]]))
    wp = []
    for c, (b, cap) in enumerate(caps):
        Rb, pb = (np.eye(3), np.asarray(d.base_pos[:])) if b < 0 else (R[b], p[b])
        wp.append((pb + Rb @ np.asarray(cap["p1"]), pb + Rb @ np.asarray(cap["p2"]), cap["r"]))
    # pre-check model (HumanEnv.check_collision_action): capsules 0..6 + the URDF's gripper cylinder = shield gripper capsule
    sc = GRIPPER["shield_capsule"]
    chk = wp[:7] + [(p[NARM - 1] + R[NARM - 1] @ (p_hand + R_hand @ np.asarray(sc[0])), p[NARM - 1] + R[NARM - 1] @ (p_hand + R_hand @ np.asarray(sc[1])), sc[2])]
    for i in range(8):
        mask = 0
        for j in range(i + 1, 8):
            bi, bj = caps[i][0], caps[j][0]
            if bi == bj or d.body_parent[bj] == bi or (bi >= 0 and d.body_parent[bi] == bj):
                continue
            if _seg_seg_dist(chk[i][0], chk[i][1], chk[j][0], chk[j][1]) - chk[i][2] - chk[j][2] < float(kw["self_collision_safety"]) + 0.005:
                continue
            mask |= 1 << j
        d.chk_selfmask[i] = mask
    for i in range(len(caps)):
        mask = 0
        for j in range(i + 1, len(caps)):
            bi, bj = caps[i][0], caps[j][0]
            if bi == bj or d.body_parent[bj] == bi or (bi >= 0 and d.body_parent[bi] == bj):
                continue
            if bi >= NARM and bj >= NARM:  # finger-finger
                continue
            if _seg_seg_dist(wp[i][0], wp[i][1], wp[j][0], wp[j][1]) - wp[i][2] - wp[j][2] < float(kw["self_collision_safety"]) + 0.005:
                continue  # (closer than the pre-check's safety distance in the home pose -> never a candidate)
            mask |= 1 << j
        d.rcap_selfmask[i] = mask
    # MuJoCo's constant inverse-weight approximations at qpos0 (mj_setM0 / set0): used for constraint regularisation
    R0, p0 = robot_fk_numpy(d, np.zeros(NV))
    Jv, Jw = np.zeros((NV, 3, NV)), np.zeros((NV, 3, NV))
    M0 = np.zeros((NV, NV))
    for b in range(NV):
        com = p0[b] + R0[b] @ np.asarray(d.body_com[b][:])
        k = b
        while k >= 0:
            ax = R0[k] @ np.asarray(d.jnt_axis[k][:])
            if d.jnt_type[k] == 0:
                Jw[b][:, k] = ax
                Jv[b][:, k] = np.cross(ax, com - p0[k])
            else:
                Jv[b][:, k] = ax
            k = d.body_parent[k]
        I = np.asarray(d.body_inertia[b][:])
        Ib = np.array([[I[0], I[3], I[4]], [I[3], I[1], I[5]], [I[4], I[5], I[2]]])
        M0 += d.body_mass[b] * Jv[b].T @ Jv[b] + Jw[b].T @ (R0[b] @ Ib @ R0[b].T) @ Jw[b]
    M0 += np.diag([d.jnt_armature[i] for i in range(NV)])
    M0inv = np.linalg.inv(M0)
    for i in range(NV):
        d.dof_invweight0[i] = float(M0inv[i, i])
        d.body_invweight0[i] = float(np.trace(Jv[i] @ M0inv @ Jv[i].T) / 3.0)
    # ---- human
    HB = A["human"]["bodies"]
    names = [b["name"] for b in HB]
    for i, b in enumerate(HB):
        d.hb_parent[i] = b["parent"]
        d.hb_depth[i] = 0 if b["parent"] < 0 else d.hb_depth[b["parent"]] + 1
        d.hb_anchor[i][:] = b["anchor"]
        d.hcap_p1[i][:] = b["capsule"]["p1"]
        d.hcap_p2[i][:] = b["capsule"]["p2"]
        d.hcap_r[i] = b["capsule"]["r"]
        if i > 0:
            assert b["joint_axes"] == [[0, 0, 1], [0, 1, 0], [1, 0, 0]], "human.xml joint order is z,y,x"
    for k, n in enumerate(HUMAN_JOINT_ELEMENTS):
        d.meas_body[k] = names.index(n)
    d.site_lhand = HUMAN_JOINT_ELEMENTS.index("L_Hand")
    d.site_rhand = HUMAN_JOINT_ELEMENTS.index("R_Hand")
    d.site_head = HUMAN_JOINT_ELEMENTS.index("Head")
    d.site_lelbow = HUMAN_JOINT_ELEMENTS.index("L_Elbow")
    d.site_relbow = HUMAN_JOINT_ELEMENTS.index("R_Elbow")
    d.human_base_quat[:] = [0.5, 0.5, 0.5, 0.5]  # scipy (x,y,z,w)=(.5,.5,.5,.5) -> (w,x,y,z), human_env.py:373
    d.base_human_pos_offset[:] = [float(x) for x in kw["base_human_pos_offset"]]
    d.human_rand[:] = [float(x) for x in kw["human_rand"]]
    # ---- controller
    fcg = dict(FAILSAFE_CONFIG)
    fcg.update(kw.get("controller_configs") or {})
    d.kp = float(fcg["kp"])
    d.kd = 2.0 * math.sqrt(d.kp) * float(fcg["damping_ratio"])
    d.act_in_min, d.act_in_max = float(fcg["input_min"]), float(fcg["input_max"])
    d.act_out_min, d.act_out_max = float(fcg["output_min"]), float(fcg["output_max"])
    lim = fcg.get("qpos_limits") or SCHUNK_QPOS_LIMITS
    for j in range(NARM):
        d.qpos_limits[0][j] = lim[0][j]
        d.qpos_limits[1][j] = lim[1][j]
        d.init_qpos[j] = 0.0  # schunk_robot.py:62-65
    d.init_noise = 0.02
    # ---- shield
    st = {"OFF": CONST["HRG_SHIELD_OFF"], "SSM": CONST["HRG_SHIELD_SSM"], "PFL": CONST["HRG_SHIELD_PFL"]}
    d.shield_type = st[kw["shield_type"]]
    for j in range(NARM):
        d.v_max_allowed[j], d.a_max_allowed[j], d.j_max_allowed[j] = sp["v_max_allowed"], sp["a_max_allowed"], sp["j_max_allowed"]
        d.v_max_ltt[j], d.a_max_ltt[j], d.j_max_ltt[j] = sp["v_max_ltt"], sp["a_max_ltt"], sp["j_max_ltt"]
    d.ltt_time_sync = int(bool(sp["ltt_time_sync"]))
    d.path_amax = (sp["a_max_allowed"] - sp["a_max_ltt"]) / sp["v_max_ltt"]
    d.path_jmax = (sp["j_max_allowed"] - sp["j_max_ltt"] - 3.0 * sp["a_max_ltt"] * d.path_amax) / sp["v_max_ltt"]
    assert d.path_amax > 0 and d.path_jmax > 0
    for c in range(NARM):
        d.scap_body[c] = c
        d.scap_p1[c][:] = links[c]["capsules"][0]["p1"]
        d.scap_p2[c][:] = links[c]["capsules"][0]["p2"]
        d.scap_r[c] = links[c]["capsules"][0]["r"]
    sc = GRIPPER["shield_capsule"]
    d.scap_body[NARM] = NARM - 1
    d.scap_p1[NARM][:] = (p_hand + R_hand @ np.asarray(sc[0])).tolist()
    d.scap_p2[NARM][:] = (p_hand + R_hand @ np.asarray(sc[1])).tolist()
    d.scap_r[NARM] = sc[2]
    base = np.asarray(d.base_pos[:])
    for c in range(CONST["HRG_NSHIELD_RCAP"]):
        b = d.scap_body[c]
        reach = max(np.linalg.norm(p[b] + R[b] @ np.asarray(d.scap_p1[c][:]) - base), np.linalg.norm(p[b] + R[b] @ np.asarray(d.scap_p2[c][:]) - base))
        d.scap_alpha[c] = reach * (sp["a_max_allowed"] + sp["v_max_allowed"] ** 2)
    d.secure_radius = sp["secure_radius"]
    # fail-safe target path speed: SSM / OFF brake to a stop.  PFL brakes to the path speed at which no link point can move faster than pfl_v_safe ON THE
    # TRAJECTORY PLANNED: |v_point| <= s' sum_j |dq_j/ds| r_j with r_j = reach of everything downstream of joint j (lever arm; a model constant), evaluated
    # every cycle in the steppers -- an arm that already moves slowly keeps its own speed
    d.failsafe_sdot = 0.0
    d.pfl_v_safe = float(sp["pfl_v_safe"])
    for j in range(NARM):
        rj = 0.0
        for c in range(j, CONST["HRG_NSHIELD_RCAP"]):
            b = d.scap_body[c]
            for q in (d.scap_p1[c][:], d.scap_p2[c][:]):
                rj = max(rj, float(np.linalg.norm(p[b] + R[b] @ np.asarray(q) - p[j])) + d.scap_r[c])
        d.pfl_reach[j] = rj
    d.n_bodypart = len(BODY_PARTS)
    for k, (a, b, th, vm, am, inpos) in enumerate(BODY_PARTS):
        d.bp_joint[k][:] = [HUMAN_JOINT_ELEMENTS.index(a), HUMAN_JOINT_ELEMENTS.index(b)]
        d.bp_thickness[k], d.bp_vmax[k], d.bp_amax[k], d.bp_in_pos[k] = th, vm, am, inpos
    d.n_extremity = len(EXTREMITIES)
    anchor = {b["name"]: np.asarray(b["anchor"]) for b in HB}
    for k, (prox, ch, th, vm) in enumerate(EXTREMITIES):
        d.ext_joint[k] = HUMAN_JOINT_ELEMENTS.index(prox)
        pts = [anchor[prox]] + [anchor[c] for c in ch]
        d.ext_length[k] = float(sum(np.linalg.norm(pts[i + 1] - pts[i]) for i in range(len(pts) - 1))) + 0.1
        d.ext_thickness[k], d.ext_vmax[k] = th, vm
    d.meas_err_pos, d.meas_err_vel, d.delay = sp["meas_err_pos"], sp["meas_err_vel"], sp["delay"]
    n_h = 2 * d.n_bodypart + d.n_extremity + sum(x[5] for x in BODY_PARTS)
    assert n_h <= CONST["HRG_NHCAP_MAX"], n_h
    # ---- task
    control_timestep = 1.0 / kw["control_freq"]
    d.n_cycles = int(control_timestep / kw["control_sample_time"])  # human_env.py:503
    d.horizon = int(kw["horizon"])
    d.n_goals = max(int(kw["horizon"] * kw["n_goals_sampled_per_100_steps"] / 100), 1)       # reach_human_env.py:318-321
    d.n_anim_ids = max(int(kw["horizon"] * kw["n_animations_sampled_per_100_steps"] / 100), 1)  # human_env.py:379-382
    d.n_clips = int(n_clips)
    d.anim_step_length = int(1 / kw["control_sample_time"]) / kw["human_animation_freq"]  # human_env.py:1462-1465
    assert d.anim_step_length >= 1
    d.goal_dist = float(kw["goal_dist"])
    d.reward_scale = 1.0 if kw["reward_scale"] is None else float(kw["reward_scale"])
    d.task_reward = float(kw["task_reward"])
    d.collision_reward = float(kw["collision_reward"])
    d.sim_crash_reward = -10.0  # human_env.py:410
    d.reward_shaping = int(bool(kw["reward_shaping"]))
    d.done_at_collision = int(bool(kw["done_at_collision"]))
    d.done_at_success = int(bool(kw["done_at_success"]))
    d.safe_vel = float(kw["safe_vel"])
    d.collision_debounce_delay = float(kw["collision_debounce_delay"])
    # static / self collision pre-check (human_env.py:588-627, 1301-1348; reach_human_env.py:589-593)
    cp = collision_prevention
    d.cp_enabled = int(cp is not None)
    d.cp_replace_type = int((cp or {}).get("replace_type", 0))
    d.cp_n_resamples = int((cp or {}).get("n_resamples", 20))
    if not 0 <= d.cp_replace_type <= 2 or not 0 <= d.cp_n_resamples <= 64:
        raise ValueError("collision_prevention: replace_type in {0,1,2}, n_resamples <= 64")
    d.goal_check = int(bool(goal_check))
    d.self_collision_safety = float(kw["self_collision_safety"])
    d.obstacle_margin = 0.0 if task.world == "pick_place" else 0.01   # safety_margin: pick_place_human_cartesian_env.py:696-700 / reach_human_env.py:589-593
    d.base_cyl_r, d.base_cyl_z = 0.2, 0.91
    # ---- manipulation object / task (pick_place_human_cartesian_env.py:257-404, 613-708, 843-875)
    for f in range(CONST["HRG_NFINGER"]):
        d.finger_qpos_range[0][f], d.finger_qpos_range[1][f] = FINGER_QPOS_RANGE[0][f], FINGER_QPOS_RANGE[1][f]
    if reach_box and env_id != "ReachHuman":
        raise ValueError("reach_box: the smallBox object belongs to ReachHuman")   # (ReachHumanCart always steps with it)
    d.task = task.task
    if task.world == "reach" and task.block == "box":   # the ReachHuman world with its smallBox
        if env_id == "ReachHumanCart":   # the goal an end-effector position (reach_human_cartesian_env.py)
            for k in ("table_friction", "table_full_size"):   # (a settings file read without OmegaConf hands 5e-3 over as a string)
                if not _same_list(kw[k], ENV_DEFAULTS[env_id][k]):
                    raise NotImplementedError(f"{env_id}: env kwarg {k}={kw[k]!r} is not implemented by the HIP stepper (only {ENV_DEFAULTS[env_id][k]!r})")
            q0 = np.asarray(kw["init_joint_pos"], float).ravel()
            sp_ = np.asarray(kw["sampling_space"], float)
            if q0.shape != (NARM,) or sp_.shape != (2, 3):
                raise ValueError(f"{env_id}: init_joint_pos takes {NARM} joint angles, sampling_space [[x, y, z] lower, [x, y, z] upper]")
            d.init_qpos[:] = q0.tolist()   # _reset_internal (380-383)
            for c in range(2):
                d.sampling_space[c][:] = sp_[c].tolist()
        size = [0.05, 0.05, 0.05]                       # box_size of reach_human_env.py:573
        half = [0.5 * x for x in size]
        d.box_half[:] = half
        d.box_mass = 1000.0 * size[0] * size[1] * size[2]
        d.box_inertia[:] = [d.box_mass * size[0] ** 2 / 6.0] * 3
        d.box_inertia_mean = d.box_inertia[0]
        d.box_invweight_rot = 1.0 / d.box_inertia[0]
        tx, ty = kw.get("table_full_size", [1.5, 2.0, 0.05])[:2]
        bx, by = 0.5 * tx - 0.05, 0.5 * ty - 0.05       # the sampler covers the whole table (581-589)
        d.obj_bin[:] = [-bx, bx, -by, by]
        d.tgt_bin[:] = [-bx, bx, -by, by]
        d.obj_z = d.tgt_z = 0.8 + half[2]
        d.n_obj_placements = d.n_targets = 1
    if task.world == "pick_place":
        d.init_qpos[:] = [0.0, 0.0, -math.pi / 2, 0.0, -math.pi / 2, math.pi / 4]   # _reset_internal, 616
        lifting = env_id == "CollaborativeLiftingCart"
        size = [float(x) for x in kw["board_full_size" if lifting else "object_full_size"]]
        if not all(x > 0 for x in size):
            raise ValueError("object_full_size must be positive")
        half = [0.5 * x for x in size]
        d.box_half[:] = half
        d.box_mass = (float(kw["board_density"]) if lifting else 1000.0) * size[0] * size[1] * size[2]   # BoxObject default density 1000 [UPSTREAM robosuite]
        inertia = [d.box_mass * (half[(a + 1) % 3] ** 2 + half[(a + 2) % 3] ** 2) / 3.0 for a in range(3)]
        if size[0] == size[1] == size[2]:                        # a cube: one value, so that the deviation from the mean is exactly zero
            inertia = [d.box_mass * size[0] ** 2 / 6.0] * 3
        d.box_inertia[:] = inertia
        d.box_inertia_mean = inertia[0] if inertia[0] == inertia[1] == inertia[2] else sum(inertia) / 3.0
        d.box_invweight_rot = 1.0 / inertia[0] if inertia[0] == inertia[1] == inertia[2] else sum(1.0 / x for x in inertia) / 3.0
        tx, ty = kw["table_full_size"][0], kw["table_full_size"][1]
        d.table_half[:] = [0.5 * tx, 0.5 * ty]
        bx, by = 0.5 * tx - 0.05, 0.5 * ty - 0.05
        d.obj_bin[:] = [bx * 0.35, bx * 0.6, by * 0.25, by * 0.45]
        d.tgt_bin[:] = [bx * 0.35, bx * 0.6, by * -0.45, by * -0.25]
        if env_id in ("HumanObjectInspectionCart", "PickPlacePointingHumanCart"):   # human_object_inspection_cartesian_env.py:695-710, pick_place_pointing_human_cartesian_env.py:419-434
            d.obj_bin[:] = [bx * 0.35, bx * 0.75, -by * 0.15, by * 0.15]
        if env_id == "RobotHumanHandoverCart":      # robot_human_handover_cartesian_env.py:750-765
            d.obj_bin[:] = [bx * 0.45, bx * 0.75, -by * 0.15, by * 0.15]
            d.object_in_human_hand_reward = float(kw["object_in_human_hand_reward"])
        if env_id == "HumanRobotHandoverCart":      # human_robot_handover_cartesian_env.py:713-730
            d.tgt_bin[:] = [bx * 0.45, bx * 0.85, -by * 0.15, by * 0.15]
        if env_id == "CollaborativeStackingCart":   # _get_default_object_bin_boundaries (1058-1073); the four cubes share box_half / box_mass / box_inertia
            d.obj_bin[:] = [bx * 0.5, bx * 0.8, -by * 0.15, by * 0.15]
            d.stack_toppled_reward = float(kw["stack_toppled_reward"])
            d.second_cube_at_target_reward = float(kw["second_cube_at_target_reward"])
            d.fourth_cube_at_target_reward = float(kw["fourth_cube_at_target_reward"])
            d.stack_weld_relpos[:] = [float(x) for x in kw["stack_weld_relpos"]]
        if env_id in ("HumanObjectInspectionCart", "HumanRobotHandoverCart"):
            d.object_at_target_reward = float(kw["object_at_target_reward"])
            d.goal_exit_tolerance = float(kw["goal_exit_tolerance"])
        # UniformRandomSampler: z = reference_pos[2] (0.8) + z_offset - bottom_offset (= -half edge) [UPSTREAM robosuite]
        if lifting:
            # _reset_internal (673): the Schunk posture whose gripper straddles the board edge (the hand frame's closing axis is vertical there)
            d.init_qpos[:] = [0.0, math.pi * 19 / 48, -math.pi / 2 - 5 * math.pi / 48, 0.0, math.pi / 2, -math.pi / 4]
            for hd in range(2):
                d.lift_anchor[hd][:] = [float(x) for x in kw["lift_anchors"][hd]]
            d.lift_grip_depth = 0.0
            d.min_balance = float(kw["min_balance"])
            d.imbalance_failure_reward = float(kw["imbalance_failure_reward"])
            d.board_released_reward = float(kw["board_released_reward"])
            # the table under the board's middle: TableArena(table_full_size (0.4, 1.5, 0.05), table_offset (1.0, 0, 0.8)), 280-284, 742-746 -- a slab one metre in front
            # of the robot, its top 0.8 m above the floor; a dropped board comes to rest on it (box-box contacts of the board with the slab)
            d.table_center[:] = [1.0, 0.0]
            d.table_top_z = 0.8
        d.obj_z = 0.8 + half[2]
        d.tgt_z = 0.8 + 0.5 * size[2] + half[2]
        d.n_obj_placements = max(int(kw["horizon"] * kw["n_object_placements_sampled_per_100_steps"] / 100), 1)
        d.n_targets = max(int(kw["horizon"] * kw["n_targets_sampled_per_100_steps"] / 100), 1)
        d.object_gripped_reward = float(kw["object_gripped_reward"])
    if task.world == "hammering":
        # diagonal of M at qpos0 over the human's 69 hinges (they are dynamic DoF of the reference's model: stat.meaninertia counts them): every body has mass 1,
        # inertia diag(1, 1, 1) and its inertial frame at the common origin (human.xml:46); a hinge carries the bodies of its subtree
        n_sub = [1] * len(HB)
        for i in range(len(HB) - 1, 0, -1):
            n_sub[HB[i]["parent"]] += n_sub[i]
        human_diag = []
        for i, b in enumerate(HB):
            for ax in b["joint_axes"]:
                lever = np.cross(np.asarray(ax, float), -np.asarray(b["anchor"], float))
                human_diag.append(n_sub[i] * (1.0 + float(lever @ lever)) + float(A["human"]["armature"]))
        _fill_hammering(d, kw, list(np.diag(M0)) + human_diag)
    # ---- Cartesian action front-end (wrappers/ik_position_delta_wrapper.py)
    d.ik_enabled = int(ik_position_delta is not None)
    ik = dict(IK_DEFAULTS)
    unknown = set(ik_position_delta or {}) - set(ik) - {"urdf_file"}
    if unknown:
        raise ValueError(f"ik_position_delta: unknown keys {sorted(unknown)}")
    ik.update({k: v for k, v in (ik_position_delta or {}).items() if k != "urdf_file"})
    d.ik_max_iter = int(ik["max_iter"])
    d.ik_action_limit = float(ik["action_limit"])
    d.ik_x_output_max = float(ik["x_output_max"])
    d.ik_residual_threshold = float(ik["residual_threshold"])
    d.ik_damping = float(ik["damping"])
    d.ik_use_pos_limits = int(ik["x_position_limits"] is not None)
    if ik["x_position_limits"] is not None:
        for a in range(3):
            d.ik_pos_limits[0][a], d.ik_pos_limits[1][a] = float(ik["x_position_limits"][0][a]), float(ik["x_position_limits"][1][a])
    d.ik_ee_offset[:] = IK_EE_OFFSET
    R_init, _ = robot_fk_numpy(d, np.concatenate([np.asarray(d.init_qpos[:]), np.zeros(NV - NARM)]))
    d.ik_target_rot[:] = R_init[NARM - 1].reshape(-1).tolist()      # orientation at init_qpos, ik_position_delta_wrapper.py:74-82
    d.seed = int(kw["seed"]) & 0xFFFFFFFFFFFFFFFF
    if robot_geometry not in ("capsule", "hull"):
        raise ValueError(f"robot_geometry {robot_geometry!r}: 'capsule' or 'hull'")
    if robot_geometry == "hull":
        hv, ho = load_robot_hulls()
        assert len(ho) == CONST["HRG_NHULL"] + 1
        d.robot_hulls = 1
        d.hull_off[:] = ho.tolist()
        d.hull_verts = hv.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        d._hull_keep = hv   # the desc points into this array: it lives as long as the desc
    return d


def _fill_hammering(d, kw, tree_M0_diag):
    """CollaborativeHammeringCart (collaborative_hammering_cartesian_env.py): board, hammer stand-in, nail, the two hand equalities, task parameters."""
    NARM, NF = CONST["HRG_NARM"], CONST["HRG_NFINGER"]
    d.init_qpos[:] = [0.0, 0.0, -math.pi / 2, 0.0, -math.pi / 2, math.pi / 4]   # _reset_internal, 720
    tx, ty = kw["table_full_size"][0], kw["table_full_size"][1]
    d.table_half[:] = [0.5 * tx, 0.5 * ty]
    size = [float(x) for x in kw["board_full_size"]]
    half = [0.5 * x for x in size]
    d.hm_board_half[:] = half
    d.hm_board_mass = 1000.0 * size[0] * size[1] * size[2]                       # BoxObject(name="board") without a density: robosuite's default 1000 (934-938)
    bi = [d.hm_board_mass * (half[(a + 1) % 3] ** 2 + half[(a + 2) % 3] ** 2) / 3.0 for a in range(3)]
    d.hm_board_inertia[:] = bi
    d.hm_board_invweight_rot = sum(1.0 / x for x in bi) / 3.0
    for hd in range(2):
        d.hm_anchor[hd][:] = [float(x) for x in kw["hammer_anchors"][hd]]
    q = np.asarray(kw["hammer_weld_relquat"], float)
    d.hm_weld_relquat[:] = (q / np.linalg.norm(q)).tolist()
    # the hammer: two boxes, inertia about the common COM in the body axes (both boxes are centred on the handle axis: no products of inertia)
    hh, hd_ = np.asarray(HAMMER["handle_half"]), np.asarray(HAMMER["head_half"])
    m1, m2 = HAMMER["handle_density"] * 8 * hh.prod(), HAMMER["head_density"] * 8 * hd_.prod()
    c1, c2 = np.zeros(3), np.array([0.0, 0.0, hh[2] + hd_[2]])
    com = (m1 * c1 + m2 * c2) / (m1 + m2)
    I = np.zeros(3)
    for mm, hb, c in ((m1, hh, c1), (m2, hd_, c2)):
        off = c - com
        for a in range(3):
            I[a] += mm * (hb[(a + 1) % 3] ** 2 + hb[(a + 2) % 3] ** 2) / 3.0 + mm * (off[(a + 1) % 3] ** 2 + off[(a + 2) % 3] ** 2)
    d.hm_hammer_mass = float(m1 + m2)
    d.hm_hammer_inertia[:] = I.tolist()
    d.hm_hammer_invweight_rot = float(np.mean(1.0 / I))
    d.hm_hammer_com[:] = com.tolist()
    G = CONST
    d.hm_geom_pos[G["HRG_HG_BOARD"]][:] = [0.0, 0.0, 0.0]
    d.hm_geom_pos[G["HRG_HG_HANDLE"]][:] = (c1 - com).tolist()
    d.hm_geom_pos[G["HRG_HG_HEAD"]][:] = (c2 - com).tolist()
    d.hm_geom_pos[G["HRG_HG_NAIL"]][:] = [0.0, 0.0, NAIL["head_dz"]]
    d.hm_geom_half[G["HRG_HG_BOARD"]][:] = half
    d.hm_geom_half[G["HRG_HG_HANDLE"]][:] = hh.tolist()
    d.hm_geom_half[G["HRG_HG_HEAD"]][:] = hd_.tolist()
    d.hm_geom_half[G["HRG_HG_NAIL"]][:] = NAIL["head_half"]
    d.hm_hammer_grip_quat[:] = [math.cos(math.pi / 4), 0.0, math.sin(math.pi / 4), 0.0]      # Rotation.from_euler("y", pi / 2), 792
    # finger positions at which the pads' inner surfaces (finger origin +- 0.01, bar axis 0.019 outboard, radius 0.008) touch the handle's faces
    pad = GRIPPER["finger_capsule"][0][1] - GRIPPER["finger_capsule"][2]
    for f in range(NF):
        sg = 1.0 if f == 0 else -1.0
        d.hm_finger_grip_qpos[f] = sg * (hh[0] - abs(GRIPPER["finger_pos"][f][1]) - pad)
    nh = NAIL["head_half"]
    d.hm_nail_mass = 1000.0 * math.pi * nh[0] ** 2 * 2 * nh[2]
    # NailSampler (946-960): z_offset = half board thickness + 0.001, on top of that the dummy's half height [UPSTREAM UniformRandomSampler]; nail_head 0.06 above
    d.hm_nail_z0 = half[2] + 0.001 + NAIL["dummy_half"] + NAIL["stem"]
    d.hm_nail_range = NAIL["range"]
    d.hm_nail_frictionloss = float(kw["nail_frictionloss"])
    d.hm_nail_fric_damping = NAIL["fric_damping"]
    d.hm_nail_invweight = 1.0 / d.hm_nail_mass + 1.0 / d.hm_board_mass
    d.hm_nail_bin[:] = [half[0] * 0.1, half[0] * 0.9, -half[1] * 0.9, half[1] * 0.9]         # _get_default_nail_sample_space_boundaries (838-853)
    d.hm_goal_tolerance = float(kw["goal_tolerance"])
    d.hammer_gripped_reward_bonus = float(kw["hammer_gripped_reward_bonus"])
    d.nail_hammered_in_reward = float(kw["nail_hammered_in_reward"])
    d.gripper_controllable = int(bool(kw["gripper_controllable"]))
    d.n_obj_placements = max(int(kw["horizon"] * kw["n_nail_placements_sampled_per_100_steps"] / 100), 1)   # 370-373
    d.n_targets = 1
    # MuJoCo's noslip post-pass: sim.model.opt.noslip_iterations = 20 in _setup_references (1161); opt.noslip_tolerance stays at MuJoCo's default 1e-6.  Its
    # convergence measure is scaled by 1 / (stat.meaninertia * nv) = 1 / trace(M(qpos0)) over the reference model's 90 DoF: robot tree 8, human hinges 69 (dynamic
    # DoF there although the stepper plays them back), board 6, nail 1, hammer 6
    d.noslip_iterations = int(kw["noslip_iterations"])
    d.noslip_tolerance = float(kw["noslip_tolerance"])
    diag = list(tree_M0_diag) + [d.hm_board_mass + d.hm_nail_mass] * 3 + list(d.hm_board_inertia[:]) + [d.hm_nail_mass] + [d.hm_hammer_mass] * 3 + list(d.hm_hammer_inertia[:])
    d.noslip_scale = 1.0 / float(np.sum(diag))


def robot_fk_numpy(d, q):
    """Body frames of the 8 moving robot bodies (host-side table building only)."""
    NV = CONST["HRG_NV"]
    R, p = [None] * NV, [None] * NV
    Rb, pb = _quat2mat(d.base_quat[:]), np.asarray(d.base_pos[:])
    for i in range(NV):
        par = d.body_parent[i]
        Rp, pp = (Rb, pb) if par < 0 else (R[par], p[par])
        Rl = Rp @ _quat2mat(d.body_quat[i][:])
        pi = pp + Rp @ np.asarray(d.body_pos[i][:])
        ax = np.asarray(d.jnt_axis[i][:])
        if d.jnt_type[i] == 0:
            c, s = math.cos(q[i]), math.sin(q[i])
            K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            R[i] = Rl @ (np.eye(3) + s * K + (1 - c) * (K @ K))
            p[i] = pi
        else:
            R[i] = Rl
            p[i] = pi + Rl @ ax * q[i]
    return R, p
