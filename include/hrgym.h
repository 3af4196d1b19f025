/* hrgym.h — C ABI of libhrgym_hip.so, the MI355X-native batched stepper for human-robot-gym's
 * ReachHuman hot path (HumanEnv.step = 25 x {mj_forward, SafetyShield.step, controller, human playback,
 * contact bookkeeping, mj_step} + observation/reward/done/info + auto-reset).
 *
 * The reference has NO C interface for this path: it reaches its native engines through two Python
 * extension modules (mujoco_py's MjSim, safety_shield_py's SafetyShield).  Each entry point below names
 * the reference call site(s) it replaces (paths relative to the reference checkout):
 *
 *   hrg_batch_create   <- robosuite.make("ReachHuman", **env_kwargs)      utils/env_util.py:21-26
 *                         + FailsafeController.__init__ / SafetyShield(...) controllers/failsafe_controller/
 *                                                                          failsafe_controller/failsafe_controller.py:113-191
 *                         + SubprocVecEnv([...]) worker spawn              utils/env_util_SB3.py:75-87
 *   hrg_batch_reset    <- VecEnv.reset -> ReachHuman.reset -> HumanEnv._reset_internal
 *                                                                          environments/manipulation/human_env.py:1604-1673
 *                                                                          environments/manipulation/reach_human_env.py:509-523
 *                         + FailsafeController.reset / SafetyShield.reset  failsafe_controller.py:204-250
 *   hrg_batch_step     <- VecEnv.step_async/step_wait -> HumanEnv.step     human_env.py:470-586
 *                         (sim.forward x2 + sim.step per cycle: 504,519,523; SafetyShield.step:
 *                          failsafe_controller.py:329; humanMeasurement: 310; newLongTermTrajectory: 300)
 *                         + ReachHuman.step goal cycling                   reach_human_env.py:383-410
 *                         + TimeLimit.step                                 wrappers/time_limit.py:31-44
 *                         + SubprocVecEnv auto-reset / terminal_observation [SB3 1.5.0]
 *   hrg_batch_contacts <- sim.data.contact[:ncon] as read by HumanEnv._collision_detection
 *                                                                          human_env.py:1082-1123
 *   hrg_batch_get_state / hrg_batch_set_state
 *                      <- HumanEnv.get/set_environment_state               human_env.py:1845-1900
 *   hrg_batch_capsules <- SafetyShield.getRobotReachCapsules / getHumanReachCapsules
 *                                                                          failsafe_controller.py:393,416
 *
 * Conventions: every function returns 0 on success or a negative hrg_status; hrg_last_error() gives the
 * message (thread local).  All `dev` pointers are device (HBM) pointers owned by the caller (e.g.
 * torch tensors' data_ptr()); `host` pointers are host memory.  A batch is bound to one HIP device, is not
 * thread-safe, and orders its work on the stream handed to each call (0 = the null stream).  A simulation
 * that diverges is not an error: the env reports done=1, reward += -10, info[HRG_INFO_SIM_CRASH]=1
 * (mirrors the MujocoException handler at human_env.py:527-546).
 */
#ifndef HRGYM_H
#define HRGYM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------ sizes */
#define HRG_NARM 6        /* Schunk LWA-4P arm hinges (robot.xml:33-58) */
#define HRG_NFINGER 2     /* RethinkValidGripper slide joints (rethink_valid_gripper.py:37-42) */
#define HRG_NV (HRG_NARM + HRG_NFINGER)
#define HRG_NHB 24        /* human bodies incl. pelvis (human.xml:45-330) */
#define HRG_NHJ 23        /* measured human joints (models/objects/human/human.py:57-81) */
#define HRG_NHQ 69        /* human hinge DoF = 23 x 3 */
#define HRG_NRCAP 10      /* robot collision capsules: link0..link6, gripper base, 2 fingers */
#define HRG_NHULL 7         /* arm links with a mesh collision geom: link0 .. link6 = robot capsules 0 .. 6 (robot.xml:29-55) */
#define HRG_NSHIELD_RCAP 7 /* robot capsules the shield tracks: 6 links + gripper */
#define HRG_NBODYPART_MAX 20 /* human body parts (capsule between two measured joints) */
#define HRG_NEXTREMITY_MAX 4 /* POS-model extremities (ball at proximal joint) */
#define HRG_NHCAP_MAX 64  /* human reach capsules over all three models (fits one wavefront) */
#define HRG_LTT_NSEG 12   /* constant-jerk segments per joint of a long-term trajectory */
#define HRG_OBS_DIM 64    /* superset of the flat observation (64 floats = one 256-byte row per env: a wavefront stores a row with one coalesced
                          *  instruction); the host selects columns by obs_keys:
                          *  [0:12] object-state  [12:18] goal_difference  [18:24] robot0_joint_pos  [24:30] robot0_joint_vel
                          *  [30:33] robot0_eef_pos  [33:39] desired_goal   (human_env.py:1483-1602, reach_human_env.py:608-666)
                          *  the cube tasks serve object_quat (x, y, z, w) in [12:16] (those columns are joint-space entries of ReachHuman only)
                          *  PickPlaceHumanCart (pick_place_human_cartesian_env.py:726-841; zero for ReachHuman):
                          *  [39] object_gripped  [40:43] vec_eef_to_object  [43:46] vec_eef_to_target  [46] gripper_aperture
                          *  [47:50] object_pos  [50:53] target_pos
                          *  both tasks: [53:55] robot0_gripper_qpos  [55:57] robot0_gripper_qvel (the scripted experts' inputs,
                          *  demonstrations/experts/pick_place_human_cart_expert.py:24-41)
                          *  [57:61] quat_eef_to_object of the handover tasks / quat_eef_to_board of CollaborativeLiftingCart (x, y, z, w;
                          *  human_robot_handover_cartesian_env.py:860-875, collaborative_lifting_cartesian_env.py:1010-1031), board_quat of
                          *  CollaborativeHammeringCart; [61] its nail_hammering_progress; [62:64] unused (zero)
                          *  ReachHumanCart (reach_human_cartesian_env.py:385-434): the ReachHuman layout with goal_difference = target - eef_pos in [12:15], desired_goal =
                          *  the goal's eef position in [33:36] ([15:18], [36:39] zero) and robot0_eef_velp in [40:43] */
#define HRG_ACT_DIM 7     /* 6 joint deltas + 1 gripper (reach_human_expert.py:82-83) */
#define HRG_INFO_DIM 14
#define HRG_NCON_MAX 24   /* contacts reported per env per substep */
#define HRG_NCON_DYN 6    /* contacts that enter the constraint solve (4 pyramid rows each) */
#define HRG_NCON_DYN_BOX 8 /* ... for tasks with the manipulation object (rows 24 + 32 still fit one wavefront) */
#define HRG_NBOXV 6       /* free-joint DoF of the manipulation object */
#define HRG_NVT (HRG_NV + HRG_NBOXV)
#define HRG_NCUBE 4       /* CollaborativeStackingCart: manipulation_object_a, manipulation_object_b, human_l_cube, human_r_cube
                           * (collaborative_stacking_cartesian_env.py:1151-1178) */
#define HRG_NV_STACK (HRG_NV + HRG_NCUBE * HRG_NBOXV) /* DoF of the stacking task's constrained system: robot tree + four free joints */
#define HRG_NCON_DYN_STACK 23 /* contacts that enter its solve: 8 + 16 + 12 + 4 x 23 = 128 constraint rows = two per lane of a wavefront */
#define HRG_NROW_STACK 128
#define HRG_NV_HAMMER 24   /* CollaborativeHammeringCart: three 8-wide blocks -- robot tree 0..7 | board 8..13, nail slide joint 14, pad | hammer 16..21, pad, pad */
#define HRG_NCON_DYN_HAMMER 14 /* contacts that enter its solve: 9 + 18 + 9 + 4 x 14 = 92 constraint rows (two per lane of a wavefront).  14: a soak of 2.4 M env steps had
                                 * more contacts at the end of 6 of them (tools/soak_hammering.py prints the histogram); the rows of 20 cost the kernel two of its five workgroups per CU */
#define HRG_NPREV_MAX 24  /* remembered robot contact pairs (edge trigger, human_env.py:1109-1121) */
#define HRG_MAX_CLIPS 16
#define HRG_MAX_LOOP 4     /* layered sines of an animation loop (utils/animation_utils.py:91-119) */

/* info columns (human_env.py:752-763 + TimeLimit + sim crash) */
enum {
  HRG_INFO_COLLISION = 0,
  HRG_INFO_COLLISION_TYPE = 1,
  HRG_INFO_N_COLLISIONS = 2,
  HRG_INFO_N_COLLISIONS_STATIC = 3,
  HRG_INFO_N_COLLISIONS_ROBOT = 4,
  HRG_INFO_N_COLLISIONS_HUMAN = 5,
  HRG_INFO_N_COLLISIONS_CRITICAL = 6,
  HRG_INFO_TIMEOUT = 7,
  HRG_INFO_FAILSAFE_INTERVENTIONS = 8,
  HRG_INFO_N_GOAL_REACHED = 9,
  HRG_INFO_TRUNCATED = 10, /* TimeLimit.truncated (time_limit.py:42) */
  HRG_INFO_SIM_CRASH = 11,
  HRG_INFO_ACTION_RESAMPLES = 12, /* CollisionPreventionWrapper.action_resamples */
  HRG_INFO_N_OBJECT_HANDED_OVER = 13, /* human_robot_handover_cartesian_env.py:507-511 */
  HRG_INFO_MAX_STACK_HEIGHT = 13      /* CollaborativeStackingCart._get_info (673-679): the same (task-specific) column */
};

/* COLLISION_TYPE flag values, human_env.py:55-77 */
enum { HRG_COL_NULL = 0, HRG_COL_ALLOWED = 1, HRG_COL_HUMAN = 2, HRG_COL_ROBOT = 4, HRG_COL_STATIC = 8, HRG_COL_HUMAN_CRIT = 16 };

/* shield types, failsafe_controller.py:23,173 */
enum { HRG_SHIELD_OFF = 0, HRG_SHIELD_SSM = 1, HRG_SHIELD_PFL = 2 };

/* geom classes used by the contact classifier (human_env.py:948-964) */
/* tasks: ReachHuman (reach_human_env.py), PickPlaceHumanCart (pick_place_human_cartesian_env.py) */
enum { HRG_TASK_REACH = 0, HRG_TASK_PICK_PLACE = 1, HRG_TASK_INSPECTION = 2 /* HumanObjectInspectionCart */,
       HRG_TASK_POINTING = 3 /* PickPlacePointingHumanCart: the target is where the human points (pick_place_pointing_human_cartesian_env.py:336-360) */,
       HRG_TASK_HANDOVER_H2R = 4 /* HumanRobotHandoverCart (human_robot_handover_cartesian_env.py) */,
       HRG_TASK_HANDOVER_R2H = 5 /* RobotHumanHandoverCart (robot_human_handover_cartesian_env.py) */,
       HRG_TASK_LIFTING = 6 /* CollaborativeLiftingCart (collaborative_lifting_cartesian_env.py): robot and human carry a board together */,
       HRG_TASK_STACKING = 7 /* CollaborativeStackingCart (collaborative_stacking_cartesian_env.py): human and robot build a stack of four cubes in turns */,
       HRG_TASK_REACH_BOX = 8 /* ReachHuman with its free `smallBox` object (reach_human_env.py:573-579, 5 cm cube placed anywhere on the table; not whitelisted: a
                               * robot contact with it is a static collision); task logic of ReachHuman, stepped by the cube kernel */,
       HRG_TASK_HAMMERING = 9 /* CollaborativeHammeringCart (collaborative_hammering_cartesian_env.py): the robot holds a hammer and drives a nail into a board the
                               * human presents -- two free bodies (board, hammer), the nail on a slide joint of the board, a weld + a connect to the hands */,
       HRG_TASK_REACH_CART = 10 /* ReachHumanCart (reach_human_cartesian_env.py): ReachHuman's world with its smallBox, the goal an end-effector position -- the eef position of
                                 * a sampled joint goal that lies inside sampling_space; stepped by the cube kernel like HRG_TASK_REACH_BOX */ };
#define HRG_IS_HANDOVER(task) ((task) == HRG_TASK_HANDOVER_H2R || (task) == HRG_TASK_HANDOVER_R2H)
/* ObjectInspectionPhase, human_object_inspection_cartesian_env.py:43-49 */
enum { HRG_PHASE_APPROACH = 0, HRG_PHASE_READY = 1, HRG_PHASE_INSPECTION = 2, HRG_PHASE_RETREAT = 3, HRG_PHASE_COMPLETE = 4 };
/* HumanRobotHandoverPhase, human_robot_handover_cartesian_env.py:50-56 (same numbering) */
enum { HRG_PHASE_PRESENT = 1, HRG_PHASE_WAIT = 2 };
/* RobotHumanHandoverPhase, robot_human_handover_cartesian_env.py:49-55 */
enum { HRG_R2H_APPROACH = 0, HRG_R2H_REACH_OUT = 1, HRG_R2H_RETREAT = 2, HRG_R2H_COMPLETE = 3 };
/* CollaborativeStackingPhase, collaborative_stacking_cartesian_env.py:52-60 */
enum { HRG_STK_APPROACH = 0, HRG_STK_PLACE_FIRST = 1, HRG_STK_WAIT_FOR_SECOND = 2, HRG_STK_PLACE_THIRD = 3, HRG_STK_WAIT_FOR_FOURTH = 4, HRG_STK_RETREAT = 5,
       HRG_STK_COMPLETE = 6 };
/* CollaborativeHammeringPhase, collaborative_hammering_cartesian_env.py:48-53 */
enum { HRG_HM_APPROACH = 0, HRG_HM_PRESENT = 1, HRG_HM_RETREAT = 3, HRG_HM_COMPLETE = 4 };
/* free bodies / collision geoms of the hammering task: geom GEOM_BOX + g, body BODY_BOX + b (the nail's contacts act on the board's DoF and the slide joint) */
enum { HRG_HM_BOARD = 0, HRG_HM_HAMMER = 1, HRG_HM_NAIL = 2 };
enum { HRG_HG_BOARD = 0, HRG_HG_HANDLE = 1, HRG_HG_HEAD = 2, HRG_HG_NAIL = 3, HRG_HM_NGEOM = 4 };
/* cube indices of the stacking task (order of `self.objects`, 1176-1180): the robot's two cubes, then the cubes in the human's hands */
enum { HRG_CUBE_A = 0, HRG_CUBE_B = 1, HRG_CUBE_L = 2, HRG_CUBE_R = 3 };

enum { HRG_GEOM_ROBOT = 0, HRG_GEOM_HUMAN = 1, HRG_GEOM_ALLOWED = 2, HRG_GEOM_STATIC = 3 };

typedef enum {
  HRG_OK = 0,
  HRG_ERR_INVALID = -1,
  HRG_ERR_HIP = -2,
  HRG_ERR_NOMEM = -3,
  HRG_ERR_UNSUPPORTED = -4
} hrg_status;

/* ------------------------------------------------------------------------------------------ model (POD) */

/* One constant-model description: kinematic/inertial tables, collision capsules, controller and shield
 * parameters, env (task) parameters.  Plain doubles/ints so that ctypes can fill it. */
typedef struct hrg_model_desc {
  /* ---- robot tree: 8 moving bodies (link1..link6, finger_l, finger_r), each with one joint ---------- */
  double base_pos[3];           /* world pose of the robot root (link0 frame) */
  double base_quat[4];          /* (w,x,y,z) */
  double body_pos[HRG_NV][3];   /* frame offset in parent body frame */
  double body_quat[HRG_NV][4];
  int32_t body_parent[HRG_NV];  /* index of parent moving body, -1 = base */
  int32_t jnt_type[HRG_NV];     /* 0 hinge, 1 slide */
  double jnt_axis[HRG_NV][3];   /* in body frame */
  double jnt_range[HRG_NV][2];
  double jnt_damping[HRG_NV];
  double jnt_frictionloss[HRG_NV];
  double jnt_armature[HRG_NV];
  double body_mass[HRG_NV];     /* welded children already merged in */
  double body_com[HRG_NV][3];   /* in body frame */
  double body_inertia[HRG_NV][6]; /* about com, body frame: xx yy zz xy xz yz */
  double dof_invweight0[HRG_NV];  /* (M^-1)_ii at qpos0 (MuJoCo dof_invweight0) */
  double body_invweight0[HRG_NV]; /* trace(Jv M^-1 Jv')/3 of the body com at qpos0 (MuJoCo body_invweight0, translational) */
  double gravity[3];
  double eef_pos[3];            /* grip site in the link6 body frame */
  /* actuation: arm motors (robot.xml:4-9), finger position servos */
  double arm_ctrlrange[HRG_NARM][2];
  double finger_kp;
  double finger_ctrlrange[HRG_NFINGER][2];
  double finger_forcerange[2];
  double finger_init_qpos[HRG_NFINGER];
  double gripper_speed;         /* RethinkGripper.format_action step */
  /* ---- constraint solver (MuJoCo-style soft constraints) -------------------------------------------- */
  double timestep;              /* opt.timestep = control_sample_time (human_env.py:332) */
  double solref[2];             /* timeconst, dampratio */
  double solimp[5];             /* dmin dmax width midpoint power */
  double contact_margin_human;  /* human.xml:5 margin */
  double friction_static;       /* tangential friction of robot-static contacts (pyramidal) */
  int32_t solver_iters;
  double solver_tol;
  /* ---- collision capsules ---------------------------------------------------------------------------- */
  int32_t rcap_body[HRG_NRCAP]; /* moving-body index, -1 = base (link0) */
  double rcap_p1[HRG_NRCAP][3];
  double rcap_p2[HRG_NRCAP][3];
  double rcap_r[HRG_NRCAP];
  uint32_t rcap_selfmask[HRG_NRCAP]; /* bit j set: pair (i,j), j>i, is a candidate self-collision pair */
  double table_top_z, table_half[2], floor_z;
  double table_center[2];        /* x, y of the table's centre (TableArena table_offset: (0, 0) for most tasks, (1.0, 0) for CollaborativeLiftingCart, 284) */
  /* ---- human -------------------------------------------------------------------------------------------- */
  int32_t hb_parent[HRG_NHB];
  int32_t hb_depth[HRG_NHB];
  double hb_anchor[HRG_NHB][3]; /* joint anchor = site position, model frame (human.xml site pos) */
  double hcap_p1[HRG_NHB][3];   /* collision capsule, model frame */
  double hcap_p2[HRG_NHB][3];
  double hcap_r[HRG_NHB];
  int32_t meas_body[HRG_NHJ];   /* measured joint k -> human body index (human.py:57-81 order) */
  int32_t site_lhand, site_rhand, site_head; /* indices into the measured-joint list */
  int32_t site_lelbow, site_relbow;
  double human_base_quat[4];    /* (w,x,y,z) of Rotation.from_quat([.5,.5,.5,.5]) human_env.py:373 */
  double base_human_pos_offset[3];
  double human_rand[3];
  /* ---- controller (failsafe.json, schunk.json) ----------------------------------------------------- */
  double kp, kd;
  double act_in_min, act_in_max, act_out_min, act_out_max;
  double qpos_limits[2][HRG_NARM];
  double init_qpos[HRG_NARM];
  double init_noise;            /* robosuite "default" initialization noise magnitude */
  /* ---- shield (synthetic stand-ins for sara-shield's three YAML files) ----------------------------- */
  int32_t shield_type;
  int32_t ltt_time_sync;        /* 1: the joints of a long-term trajectory arrive together, each stretched to the slowest joint's duration (sara-shield's LongTermPlanner,
                                 * SURVEY.md B.3); 0: every joint runs its own time-optimal profile (rounds 1-2: A/B of what the synchronisation costs the shield) */
  double v_max_allowed[HRG_NARM], a_max_allowed[HRG_NARM], j_max_allowed[HRG_NARM];
  double v_max_ltt[HRG_NARM], a_max_ltt[HRG_NARM], j_max_ltt[HRG_NARM];
  double path_amax, path_jmax;  /* limits on s'' and s''' of fail-safe / recovery manoeuvres */
  double failsafe_sdot;         /* path speed the fail-safe manoeuvre brakes to under SSM / OFF: 0 (full stop).  PFL computes its own every cycle (pfl_* below) */
  int32_t scap_body[HRG_NSHIELD_RCAP];
  double scap_p1[HRG_NSHIELD_RCAP][3];
  double scap_p2[HRG_NSHIELD_RCAP][3];
  double scap_r[HRG_NSHIELD_RCAP];
  double scap_alpha[HRG_NSHIELD_RCAP]; /* max Cartesian acceleration bound of the capsule end points */
  double secure_radius;
  int32_t n_bodypart;
  int32_t bp_joint[HRG_NBODYPART_MAX][2]; /* measured-joint indices (proximal, distal) */
  double bp_thickness[HRG_NBODYPART_MAX];
  double bp_vmax[HRG_NBODYPART_MAX];
  double bp_amax[HRG_NBODYPART_MAX];
  int32_t bp_in_pos[HRG_NBODYPART_MAX];   /* part keeps its VEL capsule in the POS model (torso, head) */
  int32_t n_extremity;
  int32_t ext_joint[HRG_NEXTREMITY_MAX];  /* proximal measured joint */
  double ext_length[HRG_NEXTREMITY_MAX];
  double ext_thickness[HRG_NEXTREMITY_MAX];
  double ext_vmax[HRG_NEXTREMITY_MAX];
  double meas_err_pos, meas_err_vel, delay;
  /* ---- task / env (reach_human.yaml, human_env.yaml) ---------------------------------------------- */
  int32_t n_cycles;             /* int(control_timestep / control_sample_time) human_env.py:503 */
  int32_t horizon;
  int32_t n_goals;              /* reach_human_env.py:318-321 */
  int32_t n_anim_ids;           /* human_env.py:379-382 */
  int32_t n_clips;
  double anim_step_length;      /* int(1/timestep)/human_animation_freq, human_env.py:1462-1465 */
  double goal_dist, reward_scale, task_reward, collision_reward, sim_crash_reward;
  int32_t reward_shaping, done_at_collision, done_at_success;
  double safe_vel, collision_debounce_delay;
  /* ---- static / self collision pre-check of a goal configuration (HumanEnv.check_collision_action, human_env.py:588-627;
   *      collision objects of _setup_collision_objects, human_env.py:1301-1348; pinocchio_manipulator_model.py:168-236) ---- */
  int32_t cp_enabled;           /* CollisionPreventionWrapper in the stack (config/wrappers/safe.yaml) */
  int32_t cp_replace_type;      /* 0 zero action, 1 random safe action, 2 closest safe action (collision_prevention_wrapper.py:25-46) */
  int32_t cp_n_resamples;
  int32_t goal_check;           /* ReachHuman._sample_valid_pos rejects colliding goals (reach_human_env.py:525-548) */
  double self_collision_safety; /* reach_human.yaml:25 */
  double obstacle_margin;       /* safety_margin of the table / base obstacles (reach_human_env.py:589-593) */
  double base_cyl_r, base_cyl_z; /* mount pedestal cylinder (human_env.py:1333-1339) */
  uint32_t chk_selfmask[HRG_NRCAP]; /* self-collision candidates of the pre-check model: capsules 0..6 + gripper cylinder (7) */
  /* ---- manipulation object + task of PickPlaceHumanCart (pick_place_human_cartesian_env.py:257-404, 637-708) ---- */
  int32_t task;                 /* HRG_TASK_* */
  int32_t n_obj_placements, n_targets; /* max(int(horizon * n_*_sampled_per_100_steps / 100), 1): 338-349 */
  double box_half[3];           /* half extents of the box object (object_full_size / 2) */
  double box_mass, box_inertia[3]; /* BoxObject default density 1000; principal inertia m (b^2 + c^2) / 3 per axis (half extents b, c) */
  double box_inertia_mean;      /* mean of box_inertia: the rotational inertia is handled as mean * identity + R diag(inertia - mean) R' */
  double box_invweight_rot;     /* body_invweight0 (rotation) of the free body: mean of 1 / box_inertia */
  /* ---- CollaborativeLiftingCart (collaborative_lifting_cartesian_env.py) ---- */
  double lift_anchor[2][3];     /* board-frame anchors of the left / right hand grips: connect equalities to the hand mocap bodies (786-795, 924-958) */
  double lift_grip_depth;       /* how far the board's robot-side edge reaches past the grip site along the gripper axis at a reset */
  double min_balance;           /* episode ends when (board normal . world up) falls below (509-533) */
  double imbalance_failure_reward, board_released_reward; /* _sparse_reward (446-478) */
  double obj_bin[4], tgt_bin[4]; /* xmin xmax ymin ymax of the sampling bins (843-875) */
  double obj_z, tgt_z;          /* z of a sampled object centre / target (UniformRandomSampler reference_pos + z_offset) */
  double object_gripped_reward;
  double object_at_target_reward, goal_exit_tolerance; /* HumanObjectInspectionCart, human_object_inspection_cartesian_env.py:318-321 */
  double object_in_human_hand_reward; /* RobotHumanHandoverCart, robot_human_handover_cartesian_env.py:530-555 */
  double finger_qpos_range[2][HRG_NFINGER]; /* RethinkValidGripper.qpos_range, rethink_valid_gripper.py:29-42 */
  /* ---- Cartesian action front-end (IKPositionDeltaWrapper, wrappers/ik_position_delta_wrapper.py:26-142;
   *      config/wrappers/ik_position_delta/default_ik_position_delta.yaml).  When enabled an action row is
   *      [dx, dy, dz, gripper, -, -, -] and is rewritten in place to the joint action it was converted to. ---- */
  int32_t ik_enabled;
  int32_t ik_max_iter;          /* max_iter (50) */
  int32_t ik_use_pos_limits;    /* x_position_limits is not None */
  double ik_action_limit;       /* action_limit (0.15): clip of the position delta */
  double ik_x_output_max;       /* x_output_max (1) */
  double ik_residual_threshold; /* residual_threshold (1e-3) */
  double ik_damping;            /* lambda of the damped least squares step (pybullet [UPSTREAM]: stand-in 0.1) */
  double ik_pos_limits[2][3];
  double ik_ee_offset[3];       /* end-effector link origin in the link-6 frame: fixed_gripper_joint of robot_pybullet.urdf (0, 0, 0.17) */
  double ik_target_rot[9];      /* end-effector orientation at init_qpos, held fixed (ik_position_delta_wrapper.py:74-82) */
  /* ---- CollaborativeStackingCart (collaborative_stacking_cartesian_env.py:316-480): box_half / box_mass / box_inertia describe each of the four cubes ---- */
  double stack_toppled_reward, second_cube_at_target_reward, fourth_cube_at_target_reward; /* _sparse_reward (700-744) */
  /* ---- PFL (power and force limiting): the fail-safe manoeuvre brakes to the path speed at which no point of the arm moves faster than pfl_v_safe on the
   *      trajectory actually planned: s'_pfl = min(1, pfl_v_safe / sum_j |dq_j/ds| pfl_reach[j]) (demos/demo_gym_functionality_Schunk_pfl_criterion.py:1-8) ---- */
  double pfl_v_safe;            /* Cartesian speed [m/s] the arm may keep while the reachable sets intersect */
  double pfl_reach[HRG_NARM];   /* largest distance of a point of the arm downstream of joint j from that joint (lever arm of its velocity) */
  double stack_weld_relpos[3];  /* relpose of the cube <-> hand mocap welds: mocap body origin in the cube frame, "0 0.045 0" (1263-1281) */
  /* ---- CollaborativeHammeringCart (collaborative_hammering_cartesian_env.py:291-381, 889-960, 1100-1145; models/assets/objects/nail.xml) ---- */
  double hm_board_half[3], hm_board_mass, hm_board_inertia[3]; /* BoxObject "board" (934-938): board_full_size / 2, default density 1000 */
  double hm_board_invweight_rot;  /* body_invweight0 (rotation) of the board: mean of 1 / inertia */
  double hm_anchor[2][3];         /* l_anchor / r_anchor: board-frame positions of lh_grip (connect) and rh_grip (weld), 1001-1002 */
  double hm_weld_relquat[4];      /* relpose quaternion of rh_eq (w, x, y, z), 1123-1131 */
  double hm_hammer_mass, hm_hammer_inertia[3]; /* HammerObject [UPSTREAM robosuite]: stand-in of two boxes (handle, head); inertia about the COM, body axes */
  double hm_hammer_invweight_rot;
  double hm_hammer_com[3];        /* COM in the hammer's body frame (origin = middle of the handle) */
  double hm_geom_pos[HRG_HM_NGEOM][3];  /* geom centres in their body frame: board (0), handle and head relative to the hammer's COM, nail head relative to the nail_head body */
  double hm_geom_half[HRG_HM_NGEOM][3];
  double hm_hammer_grip_quat[4];  /* world orientation the hammer is put into the gripper with: Ry(90 deg), _put_hammer_into_gripper (790-812) */
  double hm_finger_grip_qpos[HRG_NFINGER]; /* finger positions at a reset: pads touching the handle (the reference closes the gripper over 100 sim steps, 795-809) */
  double hm_nail_mass;            /* nail_head_g0, cylinder r 0.02 h 0.004 at density 1000 (nail.xml:5) */
  double hm_nail_z0;              /* nail_head body origin above the board's centre at joint position 0: placement z + 0.06 (nail.xml:3, 946-960) */
  double hm_nail_range;           /* slide joint range [0, 0.06], axis (0, 0, -1) of the board (nail.xml:7) */
  double hm_nail_frictionloss, hm_nail_fric_damping; /* frictionloss 10000, solreffriction (-100, -100): reference acceleration -damping / dmax * velocity */
  double hm_nail_invweight;       /* dof_invweight0 of the slide joint */
  double hm_nail_bin[4];          /* xmin xmax ymin ymax of the nail placements on the board (838-853) */
  double hm_goal_tolerance;       /* nail counts as hammered in when 1 - progress < goal_tolerance (505-520) */
  double hammer_gripped_reward_bonus, nail_hammered_in_reward; /* _sparse_reward (522-556) */
  /* ---- MuJoCo's noslip post-pass (mj_solNoSlip [UPSTREAM]); collaborative_hammering_cartesian_env.py:1161 sets noslip_iterations = 20, no other task does ---- */
  double noslip_tolerance;        /* opt.noslip_tolerance (MuJoCo default 1e-6): the pass ends when the scaled cost improvement of a sweep falls below it */
  double noslip_scale;            /* 1 / (stat.meaninertia * nv): the scale of that improvement (mean diagonal of M at qpos0 over the stepper's real DoF) */
  int32_t gripper_controllable;   /* False: the gripper action is replaced by 'close' (486-487) */
  int32_t noslip_iterations;      /* opt.noslip_iterations: sweeps of the pass at most; 0 = off (every task but CollaborativeHammeringCart) */
  /* ---- collision geometry of the seven arm links (robot.xml:29-55: mesh geoms, which MuJoCo convexifies at compile time) ----
   * robot_hulls = 1: contacts of an arm link with the human's capsules and with the table / floor planes are those of the link's CONVEX HULL (support mapping
   * over its vertices: GJK distance to a capsule's axis, deepest vertex under a plane), and with a manipulated object's box (the cube, the lifting board, a stacking
   * cube, the hammering board / head / nail head) the hull's penetration by MPR, one contact per pair; the link's bounding capsule is then only the broadphase.
   * Accepted by every task (each kernel has a hull variant).  0: the bounding
   * capsule itself is the collision geom (rounds 1-2).  Hull vertices: body frame, hull h = vertices hull_off[h] .. hull_off[h + 1] - 1 of
   * hull_verts[.][3] (host memory, copied at create like the clip frames; compiled from the STL files by tools/compile_model.py). */
  int32_t robot_hulls;
  int32_t hull_off[HRG_NHULL + 1];
  const double* hull_verts;
  uint64_t seed;
  /* ---- ReachHumanCart (reach_human_cartesian_env.py:283, 436-465): a goal configuration is accepted when its end-effector position lies in this box ---- */
  double sampling_space[2][3];  /* [0] lower, [1] upper corner (world) */
} hrg_model_desc;

/* Human animation clips, shared by all envs of a batch.  Frame layout (doubles):
 *   [0:3] Pelvis_pos_{x,y,z}   [3:7] Pelvis_quat (x,y,z,w — scipy order, convert_bvh.py:84-101)
 *   [7:76] 69 joint angles in qpos order of human.xml (body DFS order, per body z,y,x)
 * plus per-clip info (position_offset[3], orientation_quat[4] (x,y,z,w)): animation_utils.py:50-54 */
#define HRG_FRAME_DIM 76
typedef struct hrg_clip_table {
  int32_t n_clips;
  int32_t clip_len[HRG_MAX_CLIPS];     /* frames */
  int64_t clip_offset[HRG_MAX_CLIPS];  /* first frame index into `frames` */
  double clip_pos_offset[HRG_MAX_CLIPS][3];
  double clip_quat[HRG_MAX_CLIPS][4];  /* (x,y,z,w) */
  const double* frames;                /* host pointer, [total_frames][HRG_FRAME_DIM] */
  int64_t total_frames;
  /* per-clip entries of the animation info files the collaboration tasks read (human_object_inspection_cartesian_env.py:447-459,
   * 602-652; utils/animation_utils.py:122-176); zero for clips without them */
  int32_t clip_keyframes[HRG_MAX_CLIPS][2];
  double clip_target_pos[HRG_MAX_CLIPS][3];
  int32_t clip_n_loop[HRG_MAX_CLIPS];
  double clip_loop_amp[HRG_MAX_CLIPS][HRG_MAX_LOOP];
  double clip_loop_speed[HRG_MAX_CLIPS][HRG_MAX_LOOP];
  double clip_loop_amp_std[HRG_MAX_CLIPS], clip_loop_speed_std[HRG_MAX_CLIPS];
  int32_t clip_pointing_hand[HRG_MAX_CLIPS]; /* 0 right, 1 left ("pointing_hand" of the info file) */
  /* handover clips: two loop stages ("present" uses clip_loop_*, "wait" the arrays below) and the hand that holds the object
   * (human_robot_handover_cartesian_env.py:440-463) */
  int32_t clip_holding_hand[HRG_MAX_CLIPS];  /* 0 right, 1 left ("object_holding_hand") */
  int32_t clip_n_loop2[HRG_MAX_CLIPS];
  double clip_loop2_amp[HRG_MAX_CLIPS][HRG_MAX_LOOP];
  double clip_loop2_speed[HRG_MAX_CLIPS][HRG_MAX_LOOP];
  /* stacking clips (collaborative_stacking_cartesian_env.py:512-520, 825-897): five keyframes -- pass the table / release the first cube / first waiting
   * loop starts / release the third cube / second waiting loop starts; "first_placing_hand" is stored in clip_holding_hand, the loops of
   * "wait_for_second" / "wait_for_fourth" in clip_loop_* / clip_loop2_* */
  int32_t clip_stack_keyframes[HRG_MAX_CLIPS][5];
} hrg_clip_table;

/* ------------------------------------------------------------------------- scripted experts + action imitation reward (POD) */
/* the scripted experts of demonstrations/experts/ (REGISTERED_EXPERTS, __init__.py:8-14) */
enum { HRG_EXPERT_REACH = 0           /* ReachHumanExpert (reach_human_expert.py): joint action, reads goal_difference */,
       HRG_EXPERT_PICK_PLACE = 1      /* PickPlaceHumanCartExpert (pick_place_human_cart_expert.py): PickPlaceHumanCart, CollaborativeStackingCart, both handover tasks */,
       HRG_EXPERT_LIFTING = 2         /* CollaborativeLiftingCartExpert (collaborative_lifting_cart_expert.py) */,
       HRG_EXPERT_HAMMERING = 3       /* CollaborativeHammeringCartExpert (collaborative_hammering_cart_expert.py) */,
       HRG_EXPERT_REACH_CART = 4      /* ReachHumanCartExpert (reach_human_cart_expert.py): Cartesian action, reads goal_difference[0:3]; ReachHumanCart only */ };
/* similarity functions of utils/expert_imitation_reward_utils.py */
enum { HRG_SIM_GAUSSIAN = 0 /* 2^-(delta / iota)^2 */, HRG_SIM_TANH = 1 /* 1 - tanh(tan(0.5) delta / iota) */ };
#define HRG_IMIT_DIM 8    /* floats per env of the imitation row (hrg_batch_step_imitation) */
/* columns of the imitation row; on a done step the episode columns are the finished episode's (the accumulators restart after it) */
enum { HRG_IMIT_R_IM = 0, HRG_IMIT_R_ENV = 1, HRG_IMIT_R_MOTION = 2, HRG_IMIT_R_GRIPPER = 3, HRG_IMIT_EP_IM = 4 /* sum of r_im over the episode so far */,
       HRG_IMIT_EP_ENV = 5 /* sum of r_env */, HRG_IMIT_EP_LEN = 6 /* steps */, HRG_IMIT_R_FULL = 7 /* the combined reward (= reward_dev) */ };

/* One scripted expert (its constructor arguments) and, optionally, the ActionBasedExpertImitationRewardWrapper on top of it
 * (wrappers/action_based_expert_imitation_reward_wrapper.py: the Cart form when `cartesian`, the Joint form otherwise). */
typedef struct hrg_expert_desc {
  int32_t expert;                 /* HRG_EXPERT_* */
  int32_t cartesian;              /* 1: actions are [dx, dy, dz, gripper] (the batch has the IK front-end); 0: the 7-wide joint action */
  double act_low[HRG_ACT_DIM], act_high[HRG_ACT_DIM]; /* action_space.low / high (the first four entries when cartesian) */
  double signal_to_noise_ratio;   /* 1: the expert alone; 0: Ornstein-Uhlenbeck noise alone */
  double delta_time;              /* time step of the noise process per expert call */
  uint64_t seed;                  /* keys the noise draws (with the global env id and the env's call counter) */
  /* PickPlaceHumanCartExpert (88-102) */
  double hover_dist, tan_theta, horizontal_epsilon, vertical_epsilon, goal_dist, gripper_fully_opened_threshold;
  int32_t release_when_delivered;
  /* ActionBasedExpertImitationRewardWrapper */
  int32_t reward_enabled;         /* 0: expert actions only (hrg_batch_expert_actions) */
  /* CollaborativeLiftingCartExpert (69-78) */
  double board_size[3], human_grip_offset;
  double alpha, beta, iota_m, iota_g;
  int32_t m_sim_fn, g_sim_fn;     /* HRG_SIM_* */
  int32_t normalize_joint_actions; /* Joint form: rescale both actions to [-1, 1] by the action bounds before the distance */
  int32_t reserved;
} hrg_expert_desc;

/* ------------------------------------------------------------------------- demonstration datasets: RSI + state imitation reward (POD) */
/* StateBasedExpertImitationRewardWrapper subclasses (wrappers/state_based_expert_imitation_reward_wrapper.py) */
enum { HRG_SIR_NONE = 0        /* DatasetRSIWrapper alone (dataset_wrapper.py:88-157): resets to dataset states, no state reward */,
       HRG_SIR_REACH = 1       /* ReachHumanStateBasedExpertImitationRewardWrapper (283-413): goal_difference, all six columns (ReachHumanCart: three, the rest zero) */,
       HRG_SIR_PICK_PLACE = 2  /* PickPlaceHumanCartStateBasedExpertImitationRewardWrapper (416-619): vec_eef_to_target, robot0_gripper_qpos, object_gripped */,
       HRG_SIR_LIFTING = 3     /* CollaborativeLiftingCartStateBasedExpertImitationRewardWrapper (622-758): vec_eef_to_human_lh, board_gripped */ };
#define HRG_SIR_DIM 16    /* floats per env of the state imitation row (hrg_batch_step_dataset) */
/* columns of the state imitation row; on a finished step the episode columns are the finished episode's (the accumulators restart after it) */
enum { HRG_SIR_R_IM = 0, HRG_SIR_R_ENV = 1, HRG_SIR_R_MOTION = 2, HRG_SIR_R_GRIPPER = 3 /* pick-place only; 0 elsewhere and on a gripped-mismatch step */,
       HRG_SIR_R_FULL = 4 /* the combined reward (= reward_dev) */, HRG_SIR_EP_IM = 5, HRG_SIR_EP_ENV = 6, HRG_SIR_EP_MOTION = 7, HRG_SIR_EP_GRIPPER = 8 /* episode sums */,
       HRG_SIR_EP_LEN = 9 /* steps of the episode (len(_imitation_rewards)) */,
       HRG_SIR_EP_LEN_MG = 10 /* steps that entered the motion / gripper sums (len(_gripper_imitation_rewards), 535: without the gripped-mismatch steps) */,
       HRG_SIR_EARLY = 11 /* early_termination (152) */, HRG_SIR_TIME = 12 /* _dataset_ep_step_idx / _dataset_transition_count after the step (159): the time column of the
                                                                            * step's own observation (the terminal one where the env finished) */,
       HRG_SIR_TIME_OBS = 13 /* the time column of the obs_dev row: HRG_SIR_TIME, or the new episode's start step / T where the env finished (reset(), 107) */ };

/* One demonstration dataset (episodes concatenated) + what is done with it.  The pointers are HOST memory, read by hrg_batch_dataset_attach only. */
typedef struct hrg_dataset_desc {
  int64_t n_episodes, total_T;    /* total_T = ep_offset[n_episodes]: transitions over all episodes */
  const int64_t* ep_offset;       /* [n_episodes + 1]; episode k has T_k = ep_offset[k + 1] - ep_offset[k] >= 1 transitions */
  const void* states;             /* [total_T] hrg_env_state: the state BEFORE transition t */
  const void* boxes;              /* [total_T] hrg_box_state; NULL exactly when the batch's task is ReachHuman */
  const float* obs;               /* [total_T + n_episodes][HRG_OBS_DIM]: per episode rows 0 .. T_k, row T_k the terminal observation */
  double rsi_prob;                /* DatasetRSIWrapper rsi_prob (153-157) */
  uint64_t seed;                  /* keys the episode / start step draws (with the global env id and the env's reset counter) */
  int32_t sir_kind;               /* HRG_SIR_* */
  int32_t use_et;                 /* early termination (143-152) */
  double alpha, beta, iota_m, iota_g; /* `iota` of the Reach / Lifting wrappers is iota_m */
  double et_dist;
  int32_t m_sim_fn, g_sim_fn;     /* HRG_SIM_*; `sim_fn` of the Reach / Lifting wrappers is m_sim_fn */
} hrg_dataset_desc;

/* ------------------------------------------------------------------------- hindsight experience replay on the device (POD) */
/* which columns of the observation superset are the goals (GoalEnvironmentGymWrapper, wrappers/goal_env_wrapper.py):
 * HRG_GOAL_REACH  achieved = robot0_joint_pos [18:24], desired = desired_goal [33:39], a relabelled goal = the joint positions reached
 *                 (reach_human_env.py:477-507)
 * HRG_GOAL_CUBE   achieved = [eef_pos 30:33, object_pos 47:50, object_gripped 39], desired = target_pos [50:53], a relabelled goal = the object
 *                 position reached [47:50] (pick_place_human_cartesian_env.py:574-611) */
enum { HRG_GOAL_REACH = 0, HRG_GOAL_CUBE = 1 };
/* GoalSelectionStrategy of SB3's HerReplayBuffer */
enum { HRG_HER_FUTURE = 0, HRG_HER_FINAL = 1, HRG_HER_EPISODE = 2 };
#define HRG_HER_INDEX_DIM 3 /* int64 per sample of the optional index output of hrg_her_sample: env, write counter of the transition, write counter of the
                             * transition the new goal was taken from (-1: not relabelled) */

/* One replay buffer: the ring's shape, the sampler, the reward / done rule of relabelled transitions (copied from hrg_model_desc), the action
 * rescaling of the patched HerReplayBuffer.add (wrappers/HER_buffer_add_monkey_patch.py:64-79) and the policy's view of an observation row. */
typedef struct hrg_her_desc {
  int32_t n_envs;
  int32_t capacity;               /* transitions per env; must exceed horizon */
  int32_t horizon;                /* longest episode (TimeLimit) */
  int32_t goal_kind;              /* HRG_GOAL_* */
  int32_t strategy;               /* HRG_HER_* */
  int32_t reward_shaping, done_at_success, done_at_collision;
  double her_ratio;               /* 1 - 1 / (1 + n_sampled_goal): share of the samples that are relabelled */
  uint64_t seed;                  /* keys the sampler's draws (with the sample call counter and the sample's index in its batch) */
  double goal_dist, task_reward, object_gripped_reward, collision_reward, reward_scale;
  int32_t act_dim;                /* action values the policy sees: 7 joint space, 4 with the Cartesian front-end */
  int32_t rescale_actions;        /* 1: stored actions are 2 (a - low) / (high - low) - 1, clipped to [-1, 1] */
  double act_low[HRG_ACT_DIM], act_high[HRG_ACT_DIM];
  int32_t n_obs_cols;             /* length of the policy's `observation` entry, at most HRG_OBS_DIM */
  int32_t relabel_observation;    /* 0: a relabelled sample changes its desired_goal entry only (the reference); 1: also the copy of the goal inside
                                   * observation / next_observation */
  int32_t obs_cols[HRG_OBS_DIM];  /* column of the superset behind each value of `observation` */
  int32_t n_dg_in_obs;            /* 0, or the goal's length */
  int32_t dg_in_obs[8];           /* where component j of the desired goal sits inside `observation` */
} hrg_her_desc;

/* ------------------------------------------------------------------------- the PPO rollout buffer on the device (POD) */
/* One rollout buffer: SB3's RolloutBuffer(buffer_size = n_steps, n_envs, gamma, gae_lambda) and the policy's view of an observation row. */
typedef struct hrg_rollout_desc {
  int32_t n_envs;
  int32_t n_steps;                /* slots per env (algorithm/ppo.yaml: n_steps) */
  double gamma, gae_lambda;       /* both in [0, 1]; the device computes with (float)gamma and (float)(gamma * gae_lambda) */
  int32_t act_dim;                /* action values the policy emits: 7 joint space, 4 with the Cartesian front-end */
  int32_t n_obs_cols;             /* length of the policy's observation, at most HRG_OBS_DIM */
  int32_t obs_cols[HRG_OBS_DIM];  /* column of the superset behind each value of the observation */
} hrg_rollout_desc;

/* ------------------------------------------------------------------------- the uniform replay buffer of SAC on the device (POD) */
#define HRG_REPLAY_STATS_DIM (4 + HRG_INFO_DIM) /* doubles per env of hrg_replay_stats: finished episodes, sum of their returns, sum of their lengths, sums of the info
                                                   columns of their last steps, sum of their imitation reward sums (0 without an imitation row) */
#define HRG_REPLAY_INDEX_DIM 2 /* int64 per sample of the index input / output of hrg_replay_sample: slot, env */
/* One replay buffer: SB3's ReplayBuffer(buffer_size, n_envs = n_envs, optimize_memory_usage = False, handle_timeout_termination = True) and the policy's view of
 * an observation row: the selected columns, the state imitation reward's time column, DatasetObsNormWrapper's normalisation. */
typedef struct hrg_replay_desc {
  int32_t n_envs;
  int32_t capacity;               /* slots; each holds one transition of every env: max(buffer_size / n_envs, 1), as SB3 computes it */
  int32_t act_dim;                /* action values the policy emits: 7 joint space, 4 with the Cartesian front-end */
  int32_t n_obs_cols;             /* columns of the superset in the policy's observation */
  int32_t obs_cols[HRG_OBS_DIM];  /* column of the superset behind each value of the observation */
  int32_t observe_time;           /* 1: one more value behind the columns, the time column of the state imitation reward; n_obs_cols + observe_time <= HRG_OBS_DIM */
  int32_t normalize;              /* 1: value k becomes (v - mean[k]) / std[k], computed in double, rounded to float once */
  int32_t squash;                 /* 1 (with normalize): ... tanh(squash_factor * .) before the rounding */
  double squash_factor;
  double mean[HRG_OBS_DIM];       /* the first n_obs_cols + observe_time entries are read */
  double std[HRG_OBS_DIM];        /* non-zero (the wrapper maps 0 to 1) */
  uint64_t seed;                  /* key of the sampler's draws */
} hrg_replay_desc;

/* ------------------------------------------------------------------------- the SAC learner on the device (POD) */
#define HRG_SAC_HIDDEN 64     /* hidden width the kernels cover (net_arch [64] * depth) */
#define HRG_SAC_MAX_DEPTH 3   /* hidden layers: 1 .. 3 */
#define HRG_SAC_TILE 32       /* rows of the batch per workgroup: batch_size is a multiple */
#define HRG_SAC_MAX_BATCH 256
#define HRG_SAC_MAX_POPULATION 64 /* members of a population: learners of one shape that step in the same launches (their seeds and hrg_sac_hyper rows may differ) */
#define HRG_SAC_NQ 6          /* Q columns of hrg_sac_export: Q1, Q2 on (obs, act); the targets' Q1, Q2 on (next_obs, a'); the updated Q1, Q2 on (obs, a_pi) */
/* One learner: SB3 1.5.0's SAC(MlpPolicy, net_arch = [64] * depth, use_sde = False).  The learning rate is an argument of hrg_sac_step. */
typedef struct hrg_sac_desc {
  int32_t obs_dim;                /* 1 .. HRG_OBS_DIM */
  int32_t act_dim;                /* 1 .. HRG_ACT_DIM */
  int32_t depth;                  /* hidden layers, 1 .. HRG_SAC_MAX_DEPTH */
  int32_t hidden;                 /* HRG_SAC_HIDDEN */
  int32_t batch_size;             /* a multiple of HRG_SAC_TILE, HRG_SAC_TILE .. HRG_SAC_MAX_BATCH */
  int32_t auto_ent_coef;          /* 1: the entropy coefficient is learned ("auto", "auto_<x>") */
  int32_t target_update_interval; /* the targets move after gradient step s (counted from 0) when s % target_update_interval == 0 */
  int32_t reserved_;
  double gamma;
  double tau;
  double ent_coef;                /* the fixed coefficient (auto_ent_coef = 0); the learned one starts from the log_ent_coef entry of the parameters */
  double target_entropy;
  uint64_t seed;                  /* key of the noise draws */
} hrg_sac_desc;
/* One member's row of a SAC population's hyper-parameter table (hrg_sac_population_set_hyper): what may differ between the members of one handle.  What shapes a
 * launch or the lockstep (the dimensions, depth, batch_size, target_update_interval) stays the descriptor's. */
typedef struct hrg_sac_hyper {
  double learning_rate;           /* finite, not negative */
  double gamma;                   /* in [0, 1] */
  double tau;                     /* in [0, 1] */
  double ent_coef;                /* the fixed coefficient (auto_ent_coef = 0: positive); the learned one starts from the member's log_ent_coef entry */
  double target_entropy;
  int32_t auto_ent_coef;          /* 1: this member's entropy coefficient is learned; 0: its entry gets no gradient and no Adam step */
  int32_t reserved_;
} hrg_sac_hyper;

/* ------------------------------------------------------------------------- the PPO learner on the device (POD) */
#define HRG_PPO_HIDDEN HRG_SAC_HIDDEN       /* hidden width the kernels cover */
#define HRG_PPO_MAX_DEPTH HRG_SAC_MAX_DEPTH /* hidden layers: 1 .. 3 */
#define HRG_PPO_TILE HRG_SAC_TILE           /* rows of the minibatch per workgroup: batch_size is a multiple */
#define HRG_PPO_MAX_BATCH 4096
#define HRG_PPO_MAX_POPULATION 64           /* members of a population: learners of one shape that step in the same launches (their seeds and hrg_ppo_hyper rows may differ) */
#define HRG_PPO_NDIAG 8                     /* floats of hrg_ppo_export's diag */
#define HRG_PPO_MLP_POLICY 0                /* hrg_ppo_desc.policy: SB3's "MlpPolicy", the only one covered */
/* One learner: SB3 1.5.0's PPO(MlpPolicy, use_sde = False) with net_arch = [64] * depth (separate = 0: the shared trunk) or [dict(pi = [64] * depth, vf = [64] * depth)]
 * (separate = 1).  The learning rate and the two clip ranges are arguments of hrg_ppo_step. */
typedef struct hrg_ppo_desc {
  int32_t obs_dim;                /* 1 .. HRG_OBS_DIM */
  int32_t act_dim;                /* 1 .. HRG_ACT_DIM */
  int32_t depth;                  /* hidden layers of a network, 1 .. HRG_PPO_MAX_DEPTH */
  int32_t hidden;                 /* HRG_PPO_HIDDEN */
  int32_t separate;               /* 0: one trunk under both heads; 1: a network for the policy and one for the value function */
  int32_t batch_size;             /* a multiple of HRG_PPO_TILE, HRG_PPO_TILE .. HRG_PPO_MAX_BATCH */
  int32_t rollout_size;           /* n_envs * n_steps of the rollout buffer the minibatches come from: a multiple of batch_size; 0: not known */
  int32_t normalize_advantage;
  int32_t policy;                 /* HRG_PPO_MLP_POLICY */
  int32_t use_sde;                /* refused when set */
  int32_t target_kl_set;          /* refused when set: the early stop needs a readback per minibatch */
  int32_t reserved_;
  double ent_coef, vf_coef, max_grad_norm;
  uint64_t seed;                  /* key of the noise draws */
} hrg_ppo_desc;
/* One member's row of a PPO population's hyper-parameter table (hrg_ppo_population_set_hyper): what may differ between the members of one handle.  What shapes a
 * launch or the lockstep (the dimensions, depth, separate, batch_size, rollout_size, normalize_advantage) stays the descriptor's; n_epochs is the caller's loop. */
typedef struct hrg_ppo_hyper {
  double learning_rate;           /* finite, not negative */
  double clip_range;              /* finite, positive */
  double clip_range_vf;           /* negative: the value function is not clipped */
  double ent_coef;                /* finite, not negative */
  double vf_coef;                 /* finite, not negative */
  double max_grad_norm;           /* finite, positive */
} hrg_ppo_hyper;

/* ------------------------------------------------------------------------- behaviour cloning on the device (POD) */
#define HRG_BC_MAX_BATCH 256                /* rows of a behaviour-cloning batch: a multiple of HRG_SAC_TILE, HRG_SAC_TILE .. HRG_BC_MAX_BATCH */
enum { HRG_BC_SAC = 0, HRG_BC_PPO = 1 };   /* hrg_bc_desc.kind: the learner whose actor is trained */
/* One behaviour-cloning handle: supervised steps on the actor of a lone learner, mean squared error between its deterministic action and a table's action rows.
 * The shapes and the actor's offsets are the learner's; the learning rate is an argument of hrg_bc_step. */
typedef struct hrg_bc_desc {
  int32_t kind;                   /* HRG_BC_SAC (hrg_bc_create_sac: tanh(mu), ReLU units) | HRG_BC_PPO (hrg_bc_create_ppo: mu, tanh units) */
  int32_t batch_size;             /* a multiple of HRG_SAC_TILE, HRG_SAC_TILE .. HRG_BC_MAX_BATCH */
  uint64_t seed;                  /* of the index draws */
} hrg_bc_desc;

/* ------------------------------------------------------------------------- DAgger on the device (POD) */
#define HRG_DAGGER_STATS_DIM 3              /* doubles per env of hrg_dagger_stats */
/* columns of hrg_dagger_stats: steps, steps the expert drove, sum over the steps of sum_j (a_j - label_j)^2 (the learner's action at the label's scale) */
enum { HRG_DAGGER_STEPS = 0, HRG_DAGGER_EXPERT_STEPS = 1, HRG_DAGGER_SQ_ERROR = 2 };
/* One DAgger handle: per step, the expert's label for every env's current row, the per-env draw of who drives the step, and the (view, label) pair written into a
 * caller-owned table [pinned_rows + capacity_steps * n_envs] that hrg_bc_step trains on.  kind: the learner's (HRG_BC_SAC: actions at the policy's scale [-1, 1];
 * HRG_BC_PPO: at the env's). */
typedef struct hrg_dagger_desc {
  int32_t kind;                   /* HRG_BC_SAC | HRG_BC_PPO */
  int32_t n_envs;
  int64_t env_id0;                /* global id of env 0: the draws are keyed by env_id0 + e */
  int32_t obs_dim;                /* values of the policy's view of a row, 1 .. HRG_OBS_DIM */
  int32_t act_dim;                /* values of an action, 1 .. HRG_ACT_DIM */
  int32_t capacity_steps;         /* step slots of n_envs rows each behind the pinned rows; the oldest is overwritten */
  int32_t pinned_rows;            /* rows at the head of the table that no step writes (a demonstration table) */
  uint64_t seed;                  /* of the mixing draws */
  double act_low[HRG_ACT_DIM], act_high[HRG_ACT_DIM]; /* the action space's bounds; the first act_dim are read */
} hrg_dagger_desc;

/* ------------------------------------------------------------------------- adversarial imitation on the device (POD) */
#define HRG_DISC_MAX_BATCH 256              /* rows per half of a discriminator batch: a multiple of HRG_SAC_TILE, HRG_SAC_TILE .. HRG_DISC_MAX_BATCH */
enum { HRG_DISC_REWARD_GAIL = 0, HRG_DISC_REWARD_AIRL = 1 };   /* hrg_disc_desc.reward_kind: softplus(d) = -log(1 - D) | d = logit D */
enum { HRG_DISC_RELU = 0, HRG_DISC_TANH = 1 };                 /* hrg_disc_desc.activation: the hidden units */
/* One discriminator: an MLP of a SAC critic's shape on [obs | action] whose one output is the logit d that the row is the expert's.  The learning rate is an
 * argument of hrg_disc_step, alpha of hrg_disc_reward. */
typedef struct hrg_disc_desc {
  int32_t obs_dim;                /* 1 .. HRG_OBS_DIM */
  int32_t act_dim;                /* 1 .. HRG_ACT_DIM */
  int32_t depth;                  /* hidden layers, 1 .. HRG_SAC_MAX_DEPTH */
  int32_t hidden;                 /* HRG_SAC_HIDDEN */
  int32_t batch_size;             /* B, rows per half (B expert rows and B policy rows a step): a multiple of HRG_SAC_TILE, HRG_SAC_TILE .. HRG_DISC_MAX_BATCH */
  int32_t activation;             /* HRG_DISC_RELU | HRG_DISC_TANH */
  int32_t reward_kind;            /* HRG_DISC_REWARD_GAIL | HRG_DISC_REWARD_AIRL */
  int32_t reserved_;
  uint64_t seed;                  /* of the index draws */
} hrg_disc_desc;

/* ------------------------------------------------------------------------- evaluation of deterministic policies on the device (POD) */
#define HRG_EVAL_MAX_EPISODES_PER_ENV 4096 /* the largest quota of an env: ceil(n_eval_episodes / (n_envs / n_policies)) may not exceed it */
#define HRG_EVAL_RECORD_DIM (5 + HRG_INFO_DIM) /* doubles per record of hrg_eval_export */
/* columns of a record: Monitor's return (the env's own reward), the length, the index of the finishing step since hrg_eval_begin, TimeLimit.truncated, the info
 * columns of the last step (HRG_EVAL_REC_INFO + HRG_INFO_*), the episode's sum of imitation rewards (0 without an imitation row) */
enum { HRG_EVAL_REC_RETURN = 0, HRG_EVAL_REC_LENGTH = 1, HRG_EVAL_REC_STEP = 2, HRG_EVAL_REC_TRUNCATED = 3, HRG_EVAL_REC_INFO = 4, HRG_EVAL_REC_EP_IM = 4 + HRG_INFO_DIM };
/* One evaluation: SB3 1.5.0's evaluate_policy(deterministic = True) for n_policies parameter sets at once.  The batch is n_policies groups of n_envs / n_policies
 * consecutive envs, group k stepped by parameter set k, n_eval_episodes per group; and the policy's view of an observation row: the selected columns, the state
 * imitation reward's time column, DatasetObsNormWrapper's normalisation (hrg_replay_desc's), or on a goal env the feature row achieved_goal | desired_goal |
 * observation (hrg_her_features'). */
typedef struct hrg_eval_desc {
  int32_t n_envs;
  int32_t n_policies;             /* parameter sets; divides n_envs */
  int32_t n_eval_episodes;        /* per parameter set; env e of a group of m takes (n_eval_episodes + e % m) / m of them (SB3's episode_count_targets) */
  int32_t act_dim;                /* action values the policy emits: 7 joint space, 4 with the Cartesian front-end */
  int32_t goal_env;               /* 1: the view is the feature row of a goal env (no time column, no normalisation) */
  int32_t goal_kind;              /* HRG_GOAL_* (goal_env = 1) */
  int32_t n_obs_cols;             /* columns of the superset in the policy's observation (goal_env: in its `observation` entry) */
  int32_t obs_cols[HRG_OBS_DIM];  /* column of the superset behind each value of the observation */
  int32_t observe_time;           /* 1: one more value behind the columns, the time column of the state imitation reward */
  int32_t normalize;              /* 1: value k becomes (v - mean[k]) / std[k], computed in double, rounded to float once */
  int32_t squash;                 /* 1 (with normalize): ... tanh(squash_factor * .) before the rounding */
  int32_t reserved_;
  double squash_factor;
  double mean[HRG_OBS_DIM];       /* the first n_obs_cols + observe_time entries are read */
  double std[HRG_OBS_DIM];        /* non-zero */
  double act_low[HRG_ACT_DIM], act_high[HRG_ACT_DIM]; /* the action space's bounds: SAC's actions are unscaled to them, PPO's clamped */
} hrg_eval_desc;

typedef struct hrg_eval hrg_eval;       /* opaque */
typedef struct hrg_batch hrg_batch; /* opaque */
typedef struct hrg_her hrg_her;     /* opaque */
typedef struct hrg_rollout hrg_rollout; /* opaque */
typedef struct hrg_replay hrg_replay;   /* opaque */
typedef struct hrg_sac hrg_sac;         /* opaque */
typedef struct hrg_ppo hrg_ppo;         /* opaque */
typedef struct hrg_bc hrg_bc;           /* opaque */
typedef struct hrg_dagger hrg_dagger;   /* opaque */
typedef struct hrg_disc hrg_disc;       /* opaque */

/* ----------------------------------------------------------------------------------------------- entry points */
const char* hrg_last_error(void);
const char* hrg_version(void);

/* size in bytes of one env's resident state block (for get/set_state buffers) */
size_t hrg_state_bytes(void);

/* Create n_envs environments with global ids [env_id0, env_id0+n_envs) on HIP device `device`.
 * Per-env random draws are keyed by (desc->seed, global env id, episode index), so the results do not
 * depend on how the global batch is sharded over GPUs. */
int hrg_batch_create(const hrg_model_desc* desc, const hrg_clip_table* clips, int32_t n_envs,
                     int64_t env_id0, int32_t device, hrg_batch** out);
void hrg_batch_destroy(hrg_batch* b);

/* Reset envs whose mask byte is non-zero (mask == NULL: all).  mask is a DEVICE pointer [n_envs].
 * obs_dev: float[n_envs][HRG_OBS_DIM], rows of reset envs are overwritten (others untouched). */
int hrg_batch_reset(hrg_batch* b, const uint8_t* mask_dev, float* obs_dev, void* stream);

/* One policy step of every env: n_cycles shield cycles, observation, reward, done, info, auto-reset.
 *   actions_dev  double[n_envs][HRG_ACT_DIM]  (with collision prevention on, rows are overwritten by the executed
 *                action, the wrapper's info["action"])
 *   obs_dev      float[n_envs][HRG_OBS_DIM]   (observation AFTER auto-reset where done)
 *   term_obs_dev float[n_envs][HRG_OBS_DIM]   (observation BEFORE auto-reset; may be NULL)
 *   reward_dev   float[n_envs];  done_dev uint8_t[n_envs];  info_dev int32_t[n_envs][HRG_INFO_DIM]
 * Asynchronous with respect to the host. */
int hrg_batch_step(hrg_batch* b, double* actions_dev, float* obs_dev, float* term_obs_dev,
                   float* reward_dev, uint8_t* done_dev, int32_t* info_dev, void* stream);

/* Parity hooks (synchronous, host buffers). */
/* contacts of the LAST substep of the last step: pairs_host int32[n_envs][HRG_NCON_MAX][2], ncon_host int32[n_envs] */
int hrg_batch_contacts(hrg_batch* b, int32_t* pairs_host, int32_t* ncon_host);
/* reach capsules of the last shield cycle: robot double[n_envs][HRG_NSHIELD_RCAP][7],
 * human double[n_envs][HRG_NHCAP_MAX][7] (p1,p2,r), n_human int32[n_envs] */
int hrg_batch_capsules(hrg_batch* b, double* robot_host, double* human_host, int32_t* n_human_host);
/* launch order of the NEXT step (diagnostic; no reference counterpart): order_host int32[n_envs] = the env each workgroup will step, n_busy_host = how many of
 * them (from the front) were busy in the last step -- robot contacts or a fail-safe manoeuvre.  The order never changes what an env computes, only when its wave starts
 * (busy envs first: the step kernel ends with its slowest wave). */
int hrg_batch_launch_order(hrg_batch* b, int32_t* order_host, int32_t* n_busy_host);
/* the capsule taps cost ~4 KB of HBM writes per env per shield cycle, so they are off unless enabled here */
int hrg_batch_enable_taps(hrg_batch* b, int32_t on);
int hrg_batch_get_state(hrg_batch* b, int32_t env, void* buf_host, size_t bytes);
int hrg_batch_set_state(hrg_batch* b, int32_t env, const void* buf_host, size_t bytes);
/* the manipulation object's part of the environment state (hrg_box_state, include/hrgym_state.h):
 * PickPlaceHumanCart.get/set_environment_state, pick_place_human_cartesian_env.py:946-975; zeros for ReachHuman */
/* batched form for reference-state initialisation (wrappers/dataset_wrapper.py:88-160 resets envs to dataset states):
 * states_host = n x hrg_env_state, boxes_host = n x hrg_box_state or NULL, for the envs listed in envs_host */
int hrg_batch_get_states(hrg_batch* b, const int32_t* envs_host, int32_t n, void* states_host, void* boxes_host);
int hrg_batch_set_states(hrg_batch* b, const int32_t* envs_host, int32_t n, const void* states_host, const void* boxes_host);
size_t hrg_box_bytes(void);
int hrg_batch_get_box(hrg_batch* b, int32_t env, void* buf_host, size_t bytes);
int hrg_batch_set_box(hrg_batch* b, int32_t env, const void* buf_host, size_t bytes);
/* the four cubes + task bookkeeping of CollaborativeStackingCart (hrg_stack_state, include/hrgym_state.h):
 * CollaborativeStackingCart.get/set_environment_state, collaborative_stacking_cartesian_env.py:1551-1600 */
size_t hrg_stack_bytes(void);
int hrg_batch_get_stack(hrg_batch* b, int32_t env, void* buf_host, size_t bytes);
int hrg_batch_set_stack(hrg_batch* b, int32_t env, const void* buf_host, size_t bytes);
/* board, hammer, nail + task bookkeeping of CollaborativeHammeringCart (hrg_hammer_state, include/hrgym_state.h):
 * CollaborativeHammeringCart.get/set_environment_state, collaborative_hammering_cartesian_env.py:1339-1377 */
size_t hrg_hammer_bytes(void);
int hrg_batch_get_hammer(hrg_batch* b, int32_t env, void* buf_host, size_t bytes);
int hrg_batch_set_hammer(hrg_batch* b, int32_t env, const void* buf_host, size_t bytes);
/* test tap of the hull variant (robot_hulls; oracle counterparts: hrgo_test_hull_segment / hrgo_test_hull_lowest): n queries {R[9] row-major, p[3], s1[3], s2[3], hull,
 * pad} = 152 bytes each, against the vertex table (verts_host, off_host[HRG_NHULL + 1]) -> out_host[n][10] = GJK distance hull - segment, witness on the hull 3, witness
 * on the segment 3, lowest point over a horizontal plane 3.  One wavefront per query runs the step kernel's own wave routines (csrc/hrgym_hull.h).  0 / -1. */
int hrg_test_hull_queries(const double* verts_host, const int32_t* off_host, const void* queries_host, int32_t n, double* out_host);
/* test tap of the hull - box MPR of the hull variants (no oracle counterpart: tests/hullbox_ref.py restates it; any box extents): n queries {R[9] row-major, p[3] (link pose), box centre[3],
 * box rotation[9] row-major, box half extents[3], hull, pad} = 224 bytes each -> out_host[n][9] = penetrating (1 / 0), depth, unit normal from the hull into the box 3,
 * position 3, converged (1 / 0).  One wavefront per query runs the step kernel's own MPR routine (csrc/hrgym_hull.h, mpr_hull_box_wave).  0 / -1. */
int hrg_test_hull_box_queries(const double* verts_host, const int32_t* off_host, const void* queries_host, int32_t n, double* out_host);
/* arm link hull - box pairs (robot_hulls, every task with an object) whose MPR penetration did not converge within 50 iterations and kept the capsule contact, counted over the batch's life
 * (every substep): count_host int64.  0 for a batch without hulls. */
int hrg_batch_mpr_fallbacks(hrg_batch* b, int64_t* count_host);
/* device memory of the batch's human pose table (one entry of HRG_POSE_DIM = 216 doubles per frame of its clip set, built at create): bytes_host int64.
 * 0 for the tasks whose kernels run the human tree kinematics every cycle (all but ReachHuman and CollaborativeLiftingCart).  0 / -1. */
int hrg_batch_pose_table_bytes(hrg_batch* b, int64_t* bytes_host);
/* test tap of the pose table: n queries {pos_off[3], rot_off[4] (w, x, y, z), clip, at} = 64 bytes each -> out_host[n][2][213] = the human pose at frame `at` of
 * `clip` under those episode offsets, [0] by the live tree kinematics (the offsets composed before the tree), [1] from the pose table: 24 capsules (p1, p2) | 23
 * sites.  One wavefront per query.  HRG_ERR_UNSUPPORTED for a batch without a pose table. */
int hrg_debug_pose_compare(hrg_batch* b, const void* queries_host, int32_t n, double* out_host);
/* test tap of the wave-wide helpers of the step kernels (csrc/hrgym_device.h): one wavefront over in_host[64], lane = index; the lanes whose bit of lane_mask is clear
 * branch around every helper call, so the helpers run under that EXEC mask.  out_host[HRG_WAVE_NOUT][64] = every lane's value (NaN in a lane outside lane_mask) of, row
 * by row: wave_sum (the scalar it returns; read from lane 63, so defined only with bit 63 set), row8_sum, row16_max, wave_max (as wave_sum), chain_prefix, subtree_sum,
 * fsqrt, dpp_f64 with the controls 0xB1, 0x4E (quad_perm), 0x141 (row_half_mirror), 0x140 (row_mirror), 0x111, 0x112, 0x114 (row_shr 1, 2, 4), 0x101, 0x102, 0x104
 * (row_shl 1, 2, 4), dpp_f64_rows with 0x142 under row mask 0xa (row_bcast15; rows 0, 2 undefined) and 0x143 under 0xc (row_bcast31; rows 0, 1 undefined), v_rsq_f64, the
 * seed fsqrt iterates from, and chain_prefix<true> / subtree_sum<true> (the forms without the select in front) over the input with 0.0 in the lanes >= HRG_NARM / >= HRG_NV.
 * 0 / -1. */
enum { HRG_WAVE_NOUT = 22 /* rows of out_host */ };
int hrg_debug_wave_helpers(const double* in_host, uint64_t lane_mask, double* out_host);
/* test tap of the cull box of collide and shield_step (csrc/hrgym_device.h, cull_box): one wavefront over the first n (1..16) of in_host[16][7], a capsule each as
 * p1[3] p2[3] radius (all 16 rows are copied; the rows >= n are not read) -> out_host[6] = lo[3] hi[3] of the box around the capsules, each inflated by its radius.  0 / -1. */
int hrg_debug_cull_box(const double* in_host, int32_t n, double* out_host);
/* test tap of the model constants that hrg_batch_create has the device precompute (expressions the step kernels evaluated in every substep before): out_host[2][HRG_MC_DIM],
 * [0] = the stored entries as the kernels read them, [1] = the same values as one wavefront computes them now from the kernels' own expressions, the friction rows' zero
 * position term passed in at run time so that the impedance code runs as in a substep.  Must be equal bit for bit.  Columns: HRG_MC_FRIC_D, HRG_MC_FRIC_LIM,
 * HRG_MC_FRIC_IMP: D, the limit floss / D and the impedance ([0]: solimp[0]) of the HRG_NV friction-loss rows and of the nail's slide joint (hammering); 0 for a dof
 * without friction loss.  HRG_MC_EUL_HD, HRG_MC_EUL_RHD, HRG_MC_EUL_FINGERS: the implicit joint damping of the integrator, h * damping of the HRG_NV joints, its
 * reciprocal for the two fingers, and whether both fingers are damped (1 / 0).  HRG_MC_RCAP_MID: the mid point of each of the HRG_NRCAP robot collision capsules in its
 * body's frame, [capsule][3].  0 / -1. */
enum { HRG_MC_FRIC_D = 0, HRG_MC_FRIC_LIM = HRG_NV + 1, HRG_MC_FRIC_IMP = 2 * (HRG_NV + 1), HRG_MC_EUL_HD = 3 * (HRG_NV + 1), HRG_MC_EUL_RHD = HRG_MC_EUL_HD + HRG_NV,
       HRG_MC_EUL_FINGERS = HRG_MC_EUL_RHD + 2, HRG_MC_RCAP_MID = HRG_MC_EUL_FINGERS + 1, HRG_MC_DIM = HRG_MC_RCAP_MID + 3 * HRG_NRCAP };
int hrg_debug_model_constants(hrg_batch* b, double* out_host);
/* test tap of the robot's chain kinematics (robot_chain_fk, csrc/hrgym_kernels.h) as the batch's kernel variant compiles it: n (1..64) triples q_host[n][3][HRG_NARM] of
 * arm joint angles -- the shield's current configuration, the configuration at the end of its brake, the simulation state (fingers at 0) -- one wavefront per triple ->
 * out_host[n][HRG_CFK_DIM]: HRG_CFK_KR the world rotation [HRG_NV][9] and HRG_CFK_KP the world position [HRG_NV][3] of the bodies at the simulation state, HRG_CFK_SCAP
 * the robot reach capsule end points [2][HRG_NSHIELD_RCAP][6] (p1, p2) at the first two configurations.  shield_on = 0 walks the simulation state alone, as the kernels
 * do without a shield: the HRG_CFK_SCAP block is then 0 and the first two configurations are not read.  0 / -1. */
enum { HRG_CFK_KR = 0, HRG_CFK_KP = 9 * HRG_NV, HRG_CFK_SCAP = 12 * HRG_NV, HRG_CFK_DIM = HRG_CFK_SCAP + 2 * HRG_NSHIELD_RCAP * 6 };
int hrg_debug_chain_fk(hrg_batch* b, const double* q_host, int32_t n, int32_t shield_on, double* out_host);
/* test tap of the robot - robot round of collide (csrc/hrgym_kernels.h) as the batch's kernel variant compiles it: n (1..HRG_SP_MAX) postures q_host[n][HRG_NARM] of
 * arm joint angles (fingers at 0), one wavefront per posture: the chain walk, the world-frame capsule end points, then candidate pair p (the pairs of rcap_selfmask,
 * i major, j minor) on lane p -> out_host[n][HRG_SP_DIM]: HRG_SP_CAPS the capsule end points [HRG_NRCAP][6] (p1, p2), HRG_SP_PAIRS one record of HRG_SP_PDIM
 * doubles per pair slot [HRG_SP_NPAIR]:
 *   {i, j, near, hit, dist, n 3, pos 3, hit_off, dist_off, n_off 3, pos_off 3}
 * near: the pair passed the broadphase (segment of the longer capsule against the bounding sphere of the shorter one); hit .. pos: the contact the round reports
 * (narrowphase behind the broadphase, as in the step); hit_off .. pos_off: the contact the narrowphase reports with the broadphase compiled out.  A contact that is
 * not reported and the slots past the model's pairs are 0.  0 / error code. */
enum { HRG_SP_NPAIR = 64, HRG_SP_PDIM = 19, HRG_SP_CAPS = 0, HRG_SP_PAIRS = 6 * HRG_NRCAP, HRG_SP_DIM = HRG_SP_PAIRS + HRG_SP_NPAIR * HRG_SP_PDIM, HRG_SP_MAX = 4096 };
int hrg_debug_self_pairs(hrg_batch* b, const double* q_host, int32_t n, double* out_host);
/* test tap of the primitive narrowphase (seg_seg, seg_box, cap_box_two: csrc/hrgym_device.h; box_box2: csrc/hrgym_kernels.h) as the batch's kernel variant compiles
 * the routines: n (1..HRG_NP_MAX) queries of one `kind`, queries_host[n][HRG_NP_QDIM] -> out_host[n][HRG_NP_ODIM], everything the routine returns.  Rotations are
 * unit quaternions (w, x, y, z).
 *   HRG_NP_SEGSEG  {p1 3, q1 3, p2 3, q2 3}                     -> {d^2, c1 3, c2 3}
 *   HRG_NP_SEGBOX  {p1 3, p2 3, centre 3, quat 4, half 3}        -> {d^2, on_seg 3, on_box 3}
 *   HRG_NP_CAPBOX  {p1 3, p2 3, centre 3, quat 4, half 3, r}     -> {d^2, on_seg 3, on_box 3, two, s[0] 3, b[0] 3, s[1] 3, b[1] 3}: seg_box, then cap_box_two for each end
 *                                                                   as the contact lists call it (only for a closest pair farther apart than 1e-9); the ends are 0 unless `two`
 *   HRG_NP_BOXBOX  {pa 3, qa 4, ha 3, pb 3, qb 4, hb 3}          -> {count, 4 x (pos 3, normal 3, dist)}; the contacts past `count` are 0
 * One query per lane, on as many lanes of a wavefront as the step kernels use (64 for the segment pair, 32 against a box; box - box: the stacking kernel's 6, the
 * hammering kernel's 4, the lifting kernel's 1, each with its own BB_WORK slice of LDS);
 * rotation matrices and centres go through LDS as in the step.  HRG_ERR_UNSUPPORTED for a kind the batch's variant does not compile (the ReachHuman kernels: the
 * segment pair only; box - box: the stacking, hammering and lifting kernels).  0 / error code. */
enum { HRG_NP_SEGSEG = 0, HRG_NP_SEGBOX = 1, HRG_NP_CAPBOX = 2, HRG_NP_BOXBOX = 3, HRG_NP_QDIM = 24, HRG_NP_ODIM = 32, HRG_NP_MAX = 4096 };
int hrg_debug_narrowphase(hrg_batch* b, int32_t kind, const double* queries_host, int32_t n, double* out_host);

/* HumanEnv.check_collision_action (human_env.py:588-627; called by CollisionPreventionWrapper, wrappers/collision_prevention_wrapper.py:38-51, and
 * utils/training_utils.py:362-366): would the joint-space action drive the robot into the static scene or itself?  The goal configuration the
 * controller would set for each env (current joint angles + scaled action, clipped to the joint limits) is tested with the pre-check capsule
 * model; nothing is stepped.  actions: device, [n_envs][HRG_ACT_DIM] f64 (not modified); collides: device, [n_envs] u8 (1 = collision). */
int hrg_batch_check_actions(hrg_batch* b, const double* actions_dev, uint8_t* collides_dev, void* hip_stream);

/* Scripted experts and the action-based expert imitation reward, next to the step kernel (csrc/hrgym_expert.h).
 *   hrg_batch_expert_attach   <- create_expert (utils/training_utils.py:153-174) + ActionBasedExpertImitationRewardWrapper.__init__; allocates and zeroes the
 *                                per-env buffers (noise state and call counter, expert action, similarities, episode sums).  Synchronous; never on the step path.
 *                                HRG_ERR_UNSUPPORTED when the expert does not fit the batch's task or action form.  Attaching again replaces the expert and
 *                                restarts its noise.
 *   hrg_batch_expert_actions  <- Expert.__call__ for every env (demonstrations/create_expert_dataset.py's role): obs_dev float[n_envs][HRG_OBS_DIM] (the rows a
 *                                reset / step wrote) -> actions_out_dev double[n_envs][HRG_ACT_DIM] (the first four entries when cartesian, the rest zero);
 *                                advances every env's noise process once.
 *   hrg_batch_step_imitation  <- ActionBasedExpertImitationRewardWrapper.step (70-105): the expert acts on obs_dev as the previous step / reset left it
 *                                (info["previous_expert_observation"]) and is compared with the agent's action rows BEFORE the step rewrites them; then the
 *                                unchanged step launch; then reward_dev <- r_im alpha + r_env (1 - alpha) and imit_dev float[n_envs][HRG_IMIT_DIM].
 * A batch without an attached expert answers HRG_ERR_INVALID (hrg_batch_step_imitation also when the expert was attached with reward_enabled = 0). */
int hrg_batch_expert_attach(hrg_batch* b, const hrg_expert_desc* desc);
int hrg_batch_expert_actions(hrg_batch* b, const float* obs_dev, double* actions_out_dev, void* stream);
int hrg_batch_step_imitation(hrg_batch* b, double* actions_dev, float* obs_dev, float* term_obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* info_dev,
                             float* imit_dev, void* stream);

/* Demonstration datasets on the device (csrc/hrgym_dataset.h): reference state initialisation and the state-based expert imitation reward, in two small
 * kernels behind the (unchanged) step launch.
 *   hrg_batch_snapshot        <- DatasetCollectionWrapper.step's get_environment_state (wrappers/dataset_collection_wrapper.py; training/create_expert_dataset.py):
 *                                ONE asynchronous device-to-device copy of the whole hrg_env_state array into states_out_dev [n_envs] (caller-owned device
 *                                memory), and of the hrg_box_state array into boxes_out_dev when that is non-null.  HRG_ERR_UNSUPPORTED for the stacking and
 *                                hammering batches (their state lives in further arrays).
 *   hrg_batch_dataset_attach  <- DatasetWrapper.load_dataset + DatasetRSIWrapper.__init__ / StateBasedExpertImitationRewardWrapper.__init__
 *                                (dataset_wrapper.py:35-113, state_based_expert_imitation_reward_wrapper.py:74-99): uploads the arrays once, allocates the per-env
 *                                cursor (episode, step, T), reset counter and episode sums.  Synchronous; never on the step path.  HRG_ERR_UNSUPPORTED for the
 *                                stacking and hammering batches and for a sir_kind that does not read the task's observation; HRG_ERR_INVALID for an episode
 *                                with T = 0, a broken episode table, a boxes pointer that does not fit the task.  Attaching again replaces the dataset.
 *   hrg_batch_dataset_reset   <- DatasetRSIWrapper.reset (115-135): hrg_batch_reset, then the masked envs (NULL: all) are restored to a dataset state: episode
 *                                floor(u0 n_episodes), step u1 < rsi_prob ? floor(u2 T) : 0, u = rng_u01(seed, global env id, reset counter, stream 9, 0..2);
 *                                state block, box block and observation row are copied, obs_dev rows of restored envs hold the dataset's observation.
 *   hrg_batch_step_dataset    <- DatasetRSIWrapper.step (137-151) + StateBasedExpertImitationRewardWrapper.step (115-174) + the reset of a finished env:
 *                                [expert pre kernel] -> hrg_batch_step -> [action imitation post kernel] -> state reward / ET / cursor -> restore of the finished
 *                                envs.  The bracketed kernels run when an expert with a reward is attached (then imit_dev must be non-null; otherwise it is
 *                                ignored).  term_obs_dev is REQUIRED: the policy's state of a finished env is its terminal observation; an env that only early
 *                                termination finished gets its obs_dev row copied there before the restore.  done_dev is set where ET fires.
 *                                sir_dev float[n_envs][HRG_SIR_DIM].  With sir_kind = HRG_SIR_NONE the state reward columns stay zero and reward_dev is untouched.
 *   hrg_batch_dataset_cursor  parity hook (synchronous): cursor_host int32[n_envs][3] = (episode, step, T) of every env. */
int hrg_batch_snapshot(hrg_batch* b, void* states_out_dev, void* boxes_out_dev, void* stream);
int hrg_batch_dataset_attach(hrg_batch* b, const hrg_dataset_desc* desc);
int hrg_batch_dataset_reset(hrg_batch* b, const uint8_t* mask_dev, float* obs_dev, void* stream);
int hrg_batch_step_dataset(hrg_batch* b, double* actions_dev, float* obs_dev, float* term_obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* info_dev,
                           float* imit_dev, float* sir_dev, void* stream);
int hrg_batch_dataset_cursor(hrg_batch* b, int32_t* cursor_host);

/* Hindsight experience replay on the device (csrc/hrgym_her.h): the replay buffer of SAC + HER (training/config/algorithm/sac_her.yaml; SB3's
 * HerReplayBuffer with wrappers/HER_buffer_add_monkey_patch.py) for a batch of goal envs.  Every env has a ring of `capacity` transitions in device
 * memory; whole episodes leave it, oldest first.  The entry points take raw device pointers (the tensors a step wrote, or synthetic ones), no hrg_batch.
 *   hrg_her_create     <- HerReplayBuffer.__init__: allocates and zeroes everything (synchronous; nothing is allocated later).  HRG_ERR_INVALID for
 *                         capacity <= horizon, n_envs < 1, act_dim or n_obs_cols out of range, a column outside the superset; HRG_ERR_UNSUPPORTED for an
 *                         unknown goal kind or strategy.
 *   hrg_her_observe    <- the first observation of an episode after a reset (SB3's _last_obs): for envs whose mask byte is non-zero (NULL: all) the
 *                         current row becomes obs_dev's and the transitions of the unfinished episode are discarded.
 *   hrg_her_add        <- custom_add (26-117), after a step: one transition per env -- the row before the step, the row after it (term_obs_dev where
 *                         done), the first act_dim values of the action row as the step left it (info["action"]; rescaled when rescale_actions), reward,
 *                         done, TimeLimit.truncated and collision_type of the info block.  A done flag closes the env's episode.
 *                         counts_dev (observe and add; may be NULL): int64 [n_envs], the closed transitions of every env after the call -- what
 *                         hrg_her_sample's prefix sums are made from.
 *   hrg_her_sample     <- _custom_sample_transitions (120-286), online sampling: batch_size transitions, uniform over the closed transitions of all envs;
 *                         counts_cum_dev int64 [n_envs + 1] = exclusive prefix sums of the counts (last entry: their total).  Sample k of call c draws
 *                         rng_u01(seed, c, k, stream 10, 0..2): transition, relabel (u1 < her_ratio), goal.  Outputs, float [batch_size][.]: observation
 *                         n_obs_cols, achieved_goal 6 / 7, desired_goal 6 / 3 (reach / cube), the same three of the next observation (next_desired_goal =
 *                         desired_goal), action act_dim, reward 1, done 1; index_dev int64 [batch_size][HRG_HER_INDEX_DIM] or NULL.  Relabelled samples:
 *                         reward and done of hrg_goal_reward_done; the others: the stored reward, done without timeouts.  Advances the call counter.
 *                         HRG_ERR_INVALID for batch_size < 1, null outputs, no closed transition (reads the total back: synchronises the stream).
 *   hrg_her_sample_features  the samples of hrg_her_sample -- the same draws, relabelling, reward, done and call counter: a call of either advances it -- as
 *                         the rows SB3 1.5.0's MultiInputPolicy feeds its MLPs (CombinedExtractor [UPSTREAM]: the flattened entries concatenated in
 *                         gym.spaces.Dict's alphabetical key order): features_dev / next_features_dev float [batch_size][F], F = 6 + 6 + n_obs_cols (reach) or
 *                         7 + 3 + n_obs_cols (cube), laid out achieved_goal | desired_goal | observation; action, reward, done and index_dev as above.  No
 *                         device-to-host copy and no synchronisation: the emptiness check is the caller's (hrg_her_counts, once before a run of calls); where
 *                         counts_cum_dev's total is <= 0 the kernel leaves the outputs unwritten.  HRG_ERR_INVALID for F > HRG_OBS_DIM, batch_size < 1,
 *                         null outputs.
 *   hrg_her_features   the same feature row of n_rows rows of the superset: rows_dev float [n_rows][HRG_OBS_DIM] -> out_dev float [n_rows][F].  rows_dev
 *                         NULL: the envs' current rows (SB3's _last_obs), n_rows is not read, out_dev float [n_envs][F].  HRG_ERR_INVALID for F > HRG_OBS_DIM.
 *   hrg_her_stats      synchronous: per_env_host double [n_envs][3 + HRG_INFO_DIM], since the last clear -- finished episodes, sum of their returns (the
 *                         env's own step rewards), sum of their lengths, sums of the info columns at their last steps; clear != 0 zeroes the accumulators
 *                         afterwards.  hrg_her_observe starts a masked env's running return and length again.
 *   hrg_her_counts     synchronous: counts_host int64[3] = transitions stored (closed or not), closed transitions, sample calls so far.
 *   hrg_her_export     synchronous parity hook: env's whole ring -- pre / post float [capacity][HRG_OBS_DIM], action float [capacity][act_dim], reward
 *                         float, done / truncated uint8, collision_type int32, ep_start int64, ep_len int32 [capacity] each, state int64[3] = write counter,
 *                         tail, open, cur_obs float [HRG_OBS_DIM].
 *   hrg_goal_reward_done  HumanEnv._compute_reward / _check_done (human_env.py:629-664, 835-858) of n caller-supplied rows on the current device: ag_dev
 *                         float [n][6 / 7], dg_dev float [n][6 / 3], ctype_dev int32 [n] -> reward_dev float [n], done_dev uint8 [n].  Reads the goal kind and
 *                         the reward / done parameters of desc. */
int hrg_her_create(const hrg_her_desc* desc, int32_t device, hrg_her** out);
void hrg_her_destroy(hrg_her* h);
int hrg_her_observe(hrg_her* h, const float* obs_dev, const uint8_t* mask_dev, int64_t* counts_dev, void* stream);
int hrg_her_add(hrg_her* h, const double* actions_dev, const float* obs_dev, const float* term_obs_dev, const float* reward_dev, const uint8_t* done_dev,
                const int32_t* info_dev, int64_t* counts_dev, void* stream);
int hrg_her_sample(hrg_her* h, int32_t batch_size, const int64_t* counts_cum_dev, float* observation_dev, float* achieved_goal_dev, float* desired_goal_dev,
                   float* next_observation_dev, float* next_achieved_goal_dev, float* next_desired_goal_dev, float* action_dev, float* reward_dev,
                   float* done_dev, int64_t* index_dev, void* stream);
int hrg_her_sample_features(hrg_her* h, int32_t batch_size, const int64_t* counts_cum_dev, float* features_dev, float* next_features_dev, float* action_dev,
                            float* reward_dev, float* done_dev, int64_t* index_dev, void* stream);
int hrg_her_features(hrg_her* h, const float* rows_dev, int32_t n_rows, float* out_dev, void* stream);
int hrg_her_stats(hrg_her* h, double* per_env_host, int32_t clear);
int hrg_her_counts(hrg_her* h, int64_t* counts_host);
int hrg_her_export(hrg_her* h, int32_t env, float* pre_host, float* post_host, float* action_host, float* reward_host, uint8_t* done_host,
                   uint8_t* truncated_host, int32_t* ctype_host, int64_t* ep_start_host, int32_t* ep_len_host, int64_t* state_host, float* cur_obs_host);
int hrg_goal_reward_done(const hrg_her_desc* desc, const float* ag_dev, const float* dg_dev, const int32_t* ctype_dev, int32_t n, float* reward_dev,
                         uint8_t* done_dev, void* stream);

/* The PPO rollout buffer on the device (csrc/hrgym_rollout.h): SB3's RolloutBuffer and the bookkeeping of OnPolicyAlgorithm.collect_rollouts for a batch of
 * envs (training/config/algorithm/ppo.yaml), plus the episode sums Monitor and callbacks/logging_callback.py keep on the host.  n_steps slots per env in device
 * memory.  The flat order of everything gathered or exported is SB3's swap_and_flatten: i = env * n_steps + step.  The entry points take raw device pointers
 * (the tensors a step wrote, or synthetic ones), no hrg_batch; all but create / destroy / stats / export are asynchronous on `stream`.  The write position
 * lives in the handle on the host.
 *   hrg_rollout_create   <- RolloutBuffer.__init__: allocates and zeroes everything (synchronous; nothing is allocated later).  HRG_ERR_INVALID for n_envs < 1,
 *                           n_steps < 1, n_obs_cols outside 1 .. HRG_OBS_DIM, a column outside 0 .. 63, act_dim outside 1 .. HRG_ACT_DIM, gamma or gae_lambda
 *                           outside [0, 1].
 *   hrg_rollout_view     the policy's view of n_rows rows of the observation superset: rows_dev float [n_rows][HRG_OBS_DIM] -> out_dev float
 *                           [n_rows][n_obs_cols], value k = column obs_cols[k].  rows_dev NULL: the envs' current rows (SB3's _last_obs; n_rows is then
 *                           n_envs, whatever was passed).
 *   hrg_rollout_observe  <- _last_obs = env.reset(), _last_episode_starts = True: for envs whose mask byte is non-zero (NULL: all) the current row becomes
 *                           obs_dev's, the episode_start flag 1, the running return and length 0.
 *   hrg_rollout_add      <- collect_rollouts + RolloutBuffer.add, after a step: slot `position` of every env takes the policy's view of the current (pre-step)
 *                           row, actions_dev float [n_envs][act_dim] (the policy's own output: SB3 stores the unclipped action), values_dev, log_probs_dev
 *                           float [n_envs], the env's episode_start flag, and reward_dev -- plus (float)gamma * terminal_values_dev[e] (one float32
 *                           multiply, one float32 add) where done_dev[e], info column HRG_INFO_TRUNCATED and terminal_values_dev are all non-zero / non-NULL.
 *                           Then the current row becomes obs_dev's (the row after auto-reset), the flag done_dev[e]; the running return adds reward_dev[e]
 *                           (no bootstrap term), the running length 1; on done the env's episode accumulators add 1 episode, the running return and
 *                           length and every info column, and the running pair is zeroed.  Advances the position.  HRG_ERR_INVALID on a full buffer.
 *   hrg_rollout_compute  <- compute_returns_and_advantage(last_values, dones = the flags): last_values_dev float [n_envs].  float32, in numpy's operation
 *                           order, no fused multiply-add.  HRG_ERR_INVALID before the buffer is full.
 *   hrg_rollout_get      <- _get_samples: index_dev int64 [batch_size] flat indices (repeats allowed) -> observations float [batch_size][n_obs_cols],
 *                           actions float [batch_size][act_dim], old_values, old_log_prob, advantages, returns float [batch_size].  The indices are TRUSTED to
 *                           lie in [0, n_envs * n_steps): the kernel does not check them (rollout.RolloutBuffer.get does, for caller-supplied ones).
 *                           HRG_ERR_INVALID before hrg_rollout_compute, for batch_size < 1, for a null argument.
 *   hrg_rollout_reset    <- RolloutBuffer.reset(): the position back to 0.  Current rows, flags, running returns and episode accumulators stay.
 *   hrg_rollout_stats    synchronous: per_env_host double [n_envs][3 + HRG_INFO_DIM] = finished episodes, sum of their returns, sum of their lengths, sums of
 *                           the info columns of their last steps, since the last clear; clear != 0 zeroes the accumulators afterwards.
 *   hrg_rollout_export   synchronous parity hook, every array in the flat order: observations float [n_envs * n_steps][n_obs_cols], actions float
 *                           [n_envs * n_steps][act_dim], rewards, values, log_probs, episode_starts, advantages, returns float [n_envs * n_steps], cur_obs
 *                           float [n_envs][HRG_OBS_DIM], flags float [n_envs], running return double [n_envs], running length int32 [n_envs], the
 *                           accumulators double [n_envs][3 + HRG_INFO_DIM], state int64[2] = position, 1 once computed. */
int hrg_rollout_create(const hrg_rollout_desc* desc, int32_t device, hrg_rollout** out);
void hrg_rollout_destroy(hrg_rollout* h);
int hrg_rollout_view(hrg_rollout* h, const float* rows_dev, int32_t n_rows, float* out_dev, void* stream);
int hrg_rollout_observe(hrg_rollout* h, const float* obs_dev, const uint8_t* mask_dev, void* stream);
int hrg_rollout_add(hrg_rollout* h, const float* actions_dev, const float* values_dev, const float* log_probs_dev, const float* terminal_values_dev,
                    const float* obs_dev, const float* reward_dev, const uint8_t* done_dev, const int32_t* info_dev, void* stream);
int hrg_rollout_compute(hrg_rollout* h, const float* last_values_dev, void* stream);
int hrg_rollout_get(hrg_rollout* h, const int64_t* index_dev, int32_t batch_size, float* observations_dev, float* actions_dev, float* old_values_dev,
                    float* old_log_prob_dev, float* advantages_dev, float* returns_dev, void* stream);
int hrg_rollout_reset(hrg_rollout* h);
int hrg_rollout_stats(hrg_rollout* h, double* per_env_host, int32_t clear);
int hrg_rollout_export(hrg_rollout* h, float* observations_host, float* actions_host, float* rewards_host, float* values_host, float* log_probs_host,
                       float* episode_starts_host, float* advantages_host, float* returns_host, float* cur_obs_host, float* flags_host, double* run_return_host,
                       int32_t* run_length_host, double* stats_host, int64_t* state_host);

/* The uniform replay buffer of SAC on the device (csrc/hrgym_replay.h): SB3's ReplayBuffer and the bookkeeping of OffPolicyAlgorithm._store_transition for a
 * batch of envs on flat observations (training/config_icra_2024: algorithm.name SAC, run.env_type env), plus the episode sums Monitor and the imitation wrappers'
 * _add_reward_to_info keep on the host.  Storage is time-major, [capacity][n_envs][.]; observations are stored as the policy sees them, K = n_obs_cols +
 * observe_time floats.  The entry points take raw device pointers (the tensors a step wrote, or synthetic ones), no hrg_batch; all but create / destroy / stats /
 * export / size are asynchronous on `stream`.  The write position, the `full` flag and the sample call counter live in the handle on the host.
 *   hrg_replay_create   <- ReplayBuffer.__init__: allocates and zeroes everything (synchronous; nothing is allocated later).  HRG_ERR_INVALID for n_envs < 1,
 *                          capacity < 1, n_obs_cols < 1, n_obs_cols + observe_time > HRG_OBS_DIM, a column outside 0 .. 63, act_dim outside 1 .. HRG_ACT_DIM, squash
 *                          without normalize, a std that is zero or not finite, a mean or squash_factor that is not finite; HRG_ERR_NOMEM with the number of bytes
 *                          asked for when the device has no room.
 *   hrg_replay_view     the policy's view of n_rows rows of the observation superset: rows_dev float [n_rows][HRG_OBS_DIM], time_dev float [n_rows] (needed
 *                          with observe_time, otherwise not read) -> out_dev float [n_rows][K].  rows_dev NULL: the envs' current rows and time values (SB3's
 *                          _last_obs; n_rows is then n_envs, whatever was passed).
 *   hrg_replay_observe  <- _last_obs = env.reset(): for envs whose mask byte is non-zero (NULL: all) the current row becomes obs_dev's, the current time value
 *                          time_dev's (float [n_envs]; needed with observe_time), the running return and length 0.
 *   hrg_replay_add      <- _store_transition + ReplayBuffer.add, after a step: slot `pos` of every env takes the view of the current (pre-step) row with the
 *                          current time value; as next observation the view of term_obs_dev with sir column HRG_SIR_TIME where done_dev[e], otherwise of obs_dev
 *                          with HRG_SIR_TIME_OBS; actions_dev float [n_envs][act_dim] as given (the agent's action at the policy's scale); reward_dev; done_dev;
 *                          info column HRG_INFO_TRUNCATED.  Then the current row becomes obs_dev's (the row after auto-reset) and the current time value
 *                          HRG_SIR_TIME_OBS; the running return adds the env's own reward (column HRG_SIR_R_ENV of sir_dev, HRG_IMIT_R_ENV of imit_dev, or
 *                          reward_dev without either), the running length 1; on done the env's accumulators add 1 episode, the running return and length,
 *                          every info column and the row's EP_IM column, and the running pair is zeroed.  imit_dev float [n_envs][HRG_IMIT_DIM] and sir_dev float
 *                          [n_envs][HRG_SIR_DIM] may be NULL; not both given; sir_dev is needed with observe_time.  Advances pos; at capacity it wraps and the
 *                          buffer is full.
 *   hrg_replay_sample   <- sample + _get_samples: slot = floor(u0 * upper), upper = full ? capacity : pos, env = floor(u1 * n_envs), u = rng_u01(seed, sample call
 *                          counter, index in the batch, 11, 0..1) -> observations float [batch_size][K], actions float [batch_size][act_dim], next_observations
 *                          float [batch_size][K], dones float [batch_size] = done * (1 - timeout), rewards float [batch_size].  index_in_dev int64
 *                          [batch_size][HRG_REPLAY_INDEX_DIM] (slot, env) replaces the draws when non-NULL (clamped to the stored slots; the call counter does not
 *                          move); index_out_dev, when non-NULL, records the pairs.  HRG_ERR_INVALID for an empty buffer, batch_size < 1, a null output.
 *   hrg_replay_stats    synchronous: per_env_host double [n_envs][HRG_REPLAY_STATS_DIM], since the last clear; clear != 0 zeroes the accumulators afterwards.
 *   hrg_replay_export   synchronous parity hook, the arrays as stored: observations, next_observations float [capacity][n_envs][K], actions float
 *                          [capacity][n_envs][act_dim], rewards float, dones, timeouts uint8 [capacity][n_envs], cur_obs float [n_envs][HRG_OBS_DIM], cur_time
 *                          float [n_envs], running return double [n_envs], running length int32 [n_envs], the accumulators, state int64[3] = pos, full, sample calls.
 *   hrg_replay_size     size_host int64[4] = pos, full, sample calls so far, bytes of device memory the buffer holds. */
int hrg_replay_create(const hrg_replay_desc* desc, int32_t device, hrg_replay** out);
void hrg_replay_destroy(hrg_replay* h);
int hrg_replay_view(hrg_replay* h, const float* rows_dev, const float* time_dev, int32_t n_rows, float* out_dev, void* stream);
int hrg_replay_observe(hrg_replay* h, const float* obs_dev, const float* time_dev, const uint8_t* mask_dev, void* stream);
int hrg_replay_add(hrg_replay* h, const float* actions_dev, const float* obs_dev, const float* term_obs_dev, const float* reward_dev, const uint8_t* done_dev,
                   const int32_t* info_dev, const float* imit_dev, const float* sir_dev, void* stream);
int hrg_replay_sample(hrg_replay* h, int32_t batch_size, const int64_t* index_in_dev, float* observations_dev, float* actions_dev, float* next_observations_dev,
                      float* dones_dev, float* rewards_dev, int64_t* index_out_dev, void* stream);
int hrg_replay_stats(hrg_replay* h, double* per_env_host, int32_t clear);
int hrg_replay_export(hrg_replay* h, float* observations_host, float* next_observations_host, float* actions_host, float* rewards_host, uint8_t* dones_host,
                      uint8_t* timeouts_host, float* cur_obs_host, float* cur_time_host, double* run_return_host, int32_t* run_length_host, double* stats_host,
                      int64_t* state_host);
int hrg_replay_size(hrg_replay* h, int64_t* size_host);

/* The SAC learner on the device (csrc/hrgym_sac.h): one gradient step of SB3 1.5.0's SAC.train (use_sde = False) in six launches on one stream, and the actor's
 * forward pass.  Parameters, Adam moments and target parameters are flat float32 device arrays of the caller's (layout: csrc/hrgym_sac.h; sizes: hrg_sac_sizes);
 * the handle owns the descriptor, the counters and the scratch.  Every entry selects the handle's device; hrg_sac_step and hrg_sac_act are asynchronous on `stream`.
 *   hrg_sac_create   checks the descriptor before anything is launched or allocated: HRG_ERR_UNSUPPORTED for a hidden width other than HRG_SAC_HIDDEN, a depth
 *                    outside 1 .. HRG_SAC_MAX_DEPTH, obs_dim outside 1 .. HRG_OBS_DIM, act_dim outside 1 .. HRG_ACT_DIM, a batch_size that is not a multiple of
 *                    HRG_SAC_TILE in HRG_SAC_TILE .. HRG_SAC_MAX_BATCH; HRG_ERR_INVALID for target_update_interval < 1 or values that are not finite.
 *   hrg_sac_sizes    size_host int64[6] = parameters in all (actor | critic 0 | critic 1 | log_ent_coef), of the actor, of one critic, gradient steps so far,
 *                    act calls that drew their noise, bytes of device memory held.
 *   hrg_sac_step     one gradient step on a batch of batch_size rows (the outputs of hrg_replay_sample): observations, next_observations float [B][obs_dim],
 *                    actions float [B][act_dim], dones, rewards float [B].  eps_pi_dev / eps_next_dev float [B][act_dim], when non-NULL, replace the draws.
 *                    params_dev, adam_m_dev, adam_v_dev float [n_params], target_dev float [2 n_critic] are updated in place.
 *   hrg_sac_act      actions_dev float [n][act_dim] = tanh(mu + std eps) of the actor on obs_dev float [n][obs_dim]; deterministic != 0: tanh(mu).  eps_dev float
 *                    [n][act_dim] replaces the draws when non-NULL (the call counter then does not move).
 *   hrg_sac_export   synchronous parity hook, the last step's intermediates on the host: y, logp, logp_next float [B], q float [HRG_SAC_NQ][B], grad float
 *                    [n_params] (the parameters' layout; the last entry is the coefficient's gradient, 0 when it is fixed), losses float [4] = actor_loss,
 *                    critic_loss, ent_coef_loss, the ent_coef the step used.  Any pointer may be NULL. */
int hrg_sac_create(const hrg_sac_desc* desc, int32_t device, hrg_sac** out);
void hrg_sac_destroy(hrg_sac* h);
int hrg_sac_sizes(hrg_sac* h, int64_t* size_host);
int hrg_sac_step(hrg_sac* h, const float* observations_dev, const float* actions_dev, const float* next_observations_dev, const float* dones_dev, const float* rewards_dev,
                 const float* eps_pi_dev, const float* eps_next_dev, float* params_dev, float* adam_m_dev, float* adam_v_dev, float* target_dev, double learning_rate,
                 void* stream);
int hrg_sac_act(hrg_sac* h, const float* params_dev, const float* obs_dev, int32_t n, const float* eps_dev, int32_t deterministic, float* actions_dev, void* stream);
int hrg_sac_export(hrg_sac* h, float* y_host, float* logp_host, float* logp_next_host, float* q_host, float* grad_host, float* losses_host);

/* A SAC population (csrc/hrgym_sac.h): n_members learners of one shape that differ in their seed, and where hrg_sac_population_set_hyper
 * was called in their hrg_sac_hyper rows, and take their gradient step in the same six launches.  The handle is an hrg_sac: the lone learner is the population of one member, and hrg_sac_sizes, hrg_sac_step, hrg_sac_restore and hrg_sac_destroy
 * serve both.  The counters (gradient steps, act calls) are the handle's: members step in lockstep.  Member p is, bit for bit, the lone learner of seeds[p] on the
 * same rows: its draws are keyed by its seed and the row's index in its own batch (hrg_sac_population_act: in its own group), its sums are its own.
 *   hrg_sac_population_create  hrg_sac_create with n_members seeds in place of the descriptor's (which is not read).  Before anything is allocated or launched:
 *                              HRG_ERR_UNSUPPORTED for n_members outside 1 .. HRG_SAC_MAX_POPULATION, HRG_ERR_INVALID for a null seeds table, then whatever
 *                              hrg_sac_create refuses.
 *   hrg_sac_step               on a population: every array is [n_members] times the lone learner's, member p's part at p times its size: observations
 *                              [P][B][obs_dim], ..., params_dev, adam_m_dev, adam_v_dev [P][n_params], target_dev [P][2 n_critic].
 *   hrg_sac_population_act     obs_dev float [P][n_group][obs_dim] -> actions_dev float [P][n_group][act_dim], member p's actor (params_dev [P][n_params]) on
 *                              group p; a draw's key is (seeds[p], act call count, row within the group, 13, j).  eps_dev [P][n_group][act_dim] as in hrg_sac_act,
 *                              which is this entry for one member and refuses a handle of more.
 *   hrg_sac_population_export  hrg_sac_export of one member; HRG_ERR_INVALID for a member outside the population.
 *   hrg_sac_population_set_hyper  the members' hyper-parameters: rows_host hrg_sac_hyper [n_members] (host memory, read before the entry returns) into the handle's
 *                              device table, which the step kernels read by member.  Without a call every row holds the descriptor's gamma, tau, ent_coef and
 *                              target_entropy and the learning_rate argument of hrg_sac_step; AFTER a call hrg_sac_step's learning_rate argument is not read for
 *                              this handle any more (nor checked): the table's is.  The table is ordered on the stream it was written on: the steps of one handle belong on one stream
 *                              (a caller that changes streams orders them itself and calls this entry again on the new one).  Every row is checked before anything is written, as hrg_sac_create checks the
 *                              descriptor and hrg_sac_step its argument, and gamma and tau must lie in [0, 1]: HRG_ERR_INVALID naming member and field (also for a
 *                              null table or an n_members that is not the handle's), and the table stays as it was.  The rows are written by a launch on `stream`,
 *                              behind the steps queued there and ahead of the next; it may be called between any two steps (a schedule).  Member p's arithmetic
 *                              reads row p only, in the types and the order the lone learner uses: member p is, bit for bit, the lone learner created with row
 *                              p's values. */
int hrg_sac_population_create(const hrg_sac_desc* desc, int32_t n_members, const uint64_t* seeds, int32_t device, hrg_sac** out);
int hrg_sac_population_act(hrg_sac* h, const float* params_dev, const float* obs_dev, int32_t n_group, const float* eps_dev, int32_t deterministic, float* actions_dev,
                           void* stream);
int hrg_sac_population_export(hrg_sac* h, int32_t member, float* y_host, float* logp_host, float* logp_next_host, float* q_host, float* grad_host, float* losses_host);
int hrg_sac_population_set_hyper(hrg_sac* h, const hrg_sac_hyper* rows_host, int32_t n_members, void* stream);

/* The grouped sample of the uniform replay buffer, for a population: the n_envs envs are n_groups groups of n_envs / n_groups consecutive envs, and group g's
 * batch_size samples come from its own envs: sample k draws u0, u1 = rng_u01(seeds[g], grouped call counter, k, 11, 0..1), slot = floor(u0 * upper), env =
 * g * m + floor(u1 * m) -- hrg_replay_sample's draws of a buffer of the group's m envs with seed seeds[g].  The outputs are hrg_replay_sample's with
 * [n_groups][batch_size] rows; seeds_dev uint64 [n_groups] is a DEVICE array.  The call counter is this entry's own (hrg_replay_sample's does not move).
 * HRG_ERR_INVALID for n_groups that do not divide n_envs (before anything is launched), an empty buffer, batch_size < 1, a null seeds table or output.
 * (Not under the hrg_replay_ prefix: the set of that handle's own entries is closed.) */
int hrg_sac_population_sample(hrg_replay* h, int32_t n_groups, int32_t batch_size, const uint64_t* seeds_dev, float* observations_dev, float* actions_dev,
                              float* next_observations_dev, float* dones_dev, float* rewards_dev, int64_t* index_out_dev, void* stream);

/* The PPO learner on the device (csrc/hrgym_ppo.h): one minibatch step of SB3 1.5.0's PPO.train (MlpPolicy, use_sde = False, Box actions) in four launches on one
 * stream, and the forward pass of the policy and of the value function.  Parameters and Adam moments are flat float32 device arrays of the caller's (layout:
 * csrc/hrgym_ppo.h; sizes: hrg_ppo_sizes); the handle owns the descriptor, the counters and the scratch.  Every entry selects the handle's device; hrg_ppo_step and
 * hrg_ppo_forward are asynchronous on `stream`.
 *   hrg_ppo_create   checks the descriptor before anything is launched or allocated: HRG_ERR_UNSUPPORTED for use_sde, a target_kl, a policy other than
 *                    HRG_PPO_MLP_POLICY, a hidden width other than HRG_PPO_HIDDEN, a depth outside 1 .. HRG_PPO_MAX_DEPTH, obs_dim outside 1 .. HRG_OBS_DIM, act_dim
 *                    outside 1 .. HRG_ACT_DIM, a batch_size that is not a multiple of HRG_PPO_TILE in HRG_PPO_TILE .. HRG_PPO_MAX_BATCH, a rollout_size that
 *                    batch_size does not divide (the learner takes no short last minibatch); HRG_ERR_INVALID for coefficients that are negative or not finite.
 *   hrg_ppo_sizes    size_host int64[6] = parameters in all, of one network's hidden layers, networks (1 shared, 2 separate), minibatch steps so far, forward
 *                    calls that drew their noise, bytes of device memory held.
 *   hrg_ppo_step     one minibatch step on batch_size rows (the outputs of hrg_rollout_get): observations float [B][obs_dim], actions float [B][act_dim],
 *                    old_values, old_log_prob, advantages, returns float [B].  clip_range_vf < 0: the value function is not clipped.  params_dev, adam_m_dev,
 *                    adam_v_dev float [n_params] are updated in place.
 *   hrg_ppo_forward  actions_dev float [n][act_dim] = mu + exp(log_std) eps (not clipped; deterministic != 0: mu), values_dev float [n], log_probs_dev float [n] of
 *                    the float32 actions, on obs_dev float [n][obs_dim].  eps_dev float [n][act_dim] replaces the draws when non-NULL (the call counter then does
 *                    not move).  actions_dev NULL: the values only.
 *   hrg_ppo_export   synchronous parity hook, the last step's intermediates on the host: values, log_prob, ratio float [B], grad float [n_params] (the parameters'
 *                    layout, before clipping), diag float [HRG_PPO_NDIAG] = policy_gradient_loss, value_loss, entropy_loss, loss, approx_kl, clip_fraction, std,
 *                    the gradient norm before clipping.  Any pointer may be NULL. */
int hrg_ppo_create(const hrg_ppo_desc* desc, int32_t device, hrg_ppo** out);
void hrg_ppo_destroy(hrg_ppo* h);
int hrg_ppo_sizes(hrg_ppo* h, int64_t* size_host);
int hrg_ppo_step(hrg_ppo* h, const float* observations_dev, const float* actions_dev, const float* old_values_dev, const float* old_log_prob_dev,
                 const float* advantages_dev, const float* returns_dev, float* params_dev, float* adam_m_dev, float* adam_v_dev, double learning_rate, double clip_range,
                 double clip_range_vf, void* stream);
int hrg_ppo_forward(hrg_ppo* h, const float* params_dev, const float* obs_dev, int32_t n, const float* eps_dev, int32_t deterministic, float* actions_dev,
                    float* values_dev, float* log_probs_dev, void* stream);
int hrg_ppo_export(hrg_ppo* h, float* values_host, float* log_prob_host, float* ratio_host, float* grad_host, float* diag_host);

/* A PPO population (csrc/hrgym_ppo.h): n_members learners of one shape that differ in their seed, and where hrg_ppo_population_set_hyper
 * was called in their hrg_ppo_hyper rows, and take their minibatch step in the same four launches.  The handle is an hrg_ppo: the lone learner is the population of one member, and hrg_ppo_sizes, hrg_ppo_step, hrg_ppo_restore, hrg_ppo_destroy and
 * hrg_eval_policy_ppo serve both; hrg_ppo_export is member 0's.  The counters (minibatch steps, forward calls) are the handle's: members step in lockstep, and
 * learning_rate, clip_range and clip_range_vf of a step are every member's until hrg_ppo_population_set_hyper gives each member its own.  Member p is, bit for
 * bit, the lone learner of seeds[p] (and of its row) on the same rows: its advantage
 * statistics, clip coefficient and diagnostics come from its own sums, its draws are keyed by its seed and the row's index in its own group.
 *   hrg_ppo_population_create   hrg_ppo_create with n_members seeds in place of the descriptor's (which is not read).  Before anything is allocated or launched:
 *                               HRG_ERR_UNSUPPORTED for n_members outside 1 .. HRG_PPO_MAX_POPULATION, HRG_ERR_INVALID for a null seeds table, then whatever
 *                               hrg_ppo_create refuses.
 *   hrg_ppo_step                on a population: every array is [n_members] times the lone learner's, member p's part at p times its size: observations
 *                               [P][B][obs_dim], ..., returns [P][B], params_dev, adam_m_dev, adam_v_dev [P][n_params].
 *   hrg_ppo_population_forward  obs_dev float [P][n_group][obs_dim] -> actions_dev float [P][n_group][act_dim], values_dev, log_probs_dev float [P][n_group], member
 *                               p's networks (params_dev [P][n_params]) on group p; a draw's key is (seeds[p], forward call count, row within the group, 14, j).
 *                               eps_dev [P][n_group][act_dim], deterministic and a NULL actions_dev (the values only) as in hrg_ppo_forward, which is this entry
 *                               for one member and refuses a handle of more.  HRG_ERR_INVALID for n_group < 1.
 *   hrg_ppo_population_export   hrg_ppo_export of one member; HRG_ERR_INVALID for a member outside the population.
 *   hrg_ppo_population_set_hyper  the members' hyper-parameters: rows_host hrg_ppo_hyper [n_members] (host memory, read before the entry returns) into the handle's
 *                               device table, which the step kernels read by member.  Without a call every row holds the descriptor's ent_coef, vf_coef and
 *                               max_grad_norm and the learning_rate, clip_range and clip_range_vf arguments of hrg_ppo_step; AFTER a call those three arguments of
 *                               hrg_ppo_step are not read for this handle any more (nor checked): the table's are.  The table is ordered on the stream it was written on: the
 *                               steps of one handle belong on one stream (as for hrg_sac_population_set_hyper).  Every row is checked before anything is
 *                               written, as hrg_ppo_create checks the descriptor and hrg_ppo_step its arguments: HRG_ERR_INVALID naming member and field (also for
 *                               a null table or an n_members that is not the handle's), and the table stays as it was.  The rows are written by a launch on
 *                               `stream`, behind the steps queued there and ahead of the next; it may be called between any two steps (a schedule).  Member p's
 *                               arithmetic reads row p only, in the types and the order the lone learner uses. */
int hrg_ppo_population_create(const hrg_ppo_desc* desc, int32_t n_members, const uint64_t* seeds, int32_t device, hrg_ppo** out);
int hrg_ppo_population_forward(hrg_ppo* h, const float* params_dev, const float* obs_dev, int32_t n_group, const float* eps_dev, int32_t deterministic,
                               float* actions_dev, float* values_dev, float* log_probs_dev, void* stream);
int hrg_ppo_population_export(hrg_ppo* h, int32_t member, float* values_host, float* log_prob_host, float* ratio_host, float* grad_host, float* diag_host);
int hrg_ppo_population_set_hyper(hrg_ppo* h, const hrg_ppo_hyper* rows_host, int32_t n_members, void* stream);

/* A learner's counters, for a checkpoint that is loaded into a fresh handle: Adam's bias corrections, the keys of the draws and (SAC) the phase of the target
 * update follow from them.
 *   hrg_sac_restore  gradient steps so far, act calls that drew their noise (hrg_sac_sizes' entries 3 and 4).
 *   hrg_ppo_restore  minibatch steps so far, forward calls that drew their noise (hrg_ppo_sizes' entries 3 and 4). */
int hrg_sac_restore(hrg_sac* h, uint64_t steps, uint64_t act_calls);
int hrg_ppo_restore(hrg_ppo* h, uint64_t steps, uint64_t forward_calls);

/* Behaviour cloning on the device (csrc/hrgym_bc.h): supervised pre-training of a lone learner's actor on a table of (observation, action) rows.
 * One step is two launches: rows drawn from the table (or supplied), the actor's trunk and mean head forward, the loss mean((a(obs) - action)^2) over rows and
 * components -- a = tanh(mu) for SAC, mu for PPO --, backward, then torch's Adam (eps 1e-8) on the entries the loss reaches: the actor's hidden layers and mean
 * head (SAC: actor.latent_pi.*, actor.mu.*; PPO: the shared trunk or mlp_extractor.policy_net.*, action_net.*).  Nothing else of params_dev is written, and the
 * learner handle is only read at create: its Adam moments, counters and every other parameter stay as they were.  The handle owns its step count (Adam's, and
 * the key of its draws) and its scratch; the moments bc_m_dev, bc_v_dev are the caller's float [n_params] device arrays in the parameters' layout, zero at the start.
 *   hrg_bc_create_sac  from a lone hrg_sac on `device`.  Before anything is allocated: HRG_ERR_INVALID for a null argument, a desc->kind other than HRG_BC_SAC, a
 *                      device other than the learner's; HRG_ERR_UNSUPPORTED for a population and for a batch_size that is not a multiple of HRG_SAC_TILE in
 *                      HRG_SAC_TILE .. HRG_BC_MAX_BATCH.  (hrg_bc_create_ppo: the same from a lone hrg_ppo and HRG_BC_PPO.)
 *   hrg_bc_sizes       size_host int64[4] = entries of the parameter vector a step updates, bc steps so far, parameters in all, bytes of device memory held.
 *   hrg_bc_step        one step, asynchronous on `stream`.  table_obs_dev float [n_rows][obs_dim], table_act_dev float [n_rows][act_dim]; index_in_dev int64
 *                      [batch_size] (clamped into the table) or NULL: row k of the batch is floor(u n_rows), clamped to n_rows - 1, with u = u01(seed, bc step
 *                      count, k, 15, 0).  HRG_ERR_INVALID for a null table, parameter or moment array, n_rows < 1, a learning_rate that is not finite or negative.
 *   hrg_bc_export      synchronous parity hook, the last step's: index_host int64 [batch_size], pred_host float [batch_size][act_dim] (the actor's
 *                      deterministic actions), grad_host float [n_params] (the parameters' layout; zero where the loss does not reach), loss_host float [1].  Any
 *                      pointer may be NULL. */
int hrg_bc_create_sac(const hrg_bc_desc* desc, hrg_sac* learner, int32_t device, hrg_bc** out);
int hrg_bc_create_ppo(const hrg_bc_desc* desc, hrg_ppo* learner, int32_t device, hrg_bc** out);
void hrg_bc_destroy(hrg_bc* h);
int hrg_bc_sizes(hrg_bc* h, int64_t* size_host);
int hrg_bc_step(hrg_bc* h, const float* table_obs_dev, const float* table_act_dev, int64_t n_rows, const int64_t* index_in_dev, float* params_dev, float* bc_m_dev,
                float* bc_v_dev, double learning_rate, void* stream);
int hrg_bc_export(hrg_bc* h, int64_t* index_host, float* pred_host, float* grad_host, float* loss_host);

/* DAgger on the device (csrc/hrgym_dagger.h): one launch per env step between the learner's action and the step kernel.  With c =
 * clip(expert_act[e][j], low[j], high[j]) in double, the label of env e is (float)(2 ((c - low) / (high - low)) - 1) for HRG_BC_SAC and (float)c for HRG_BC_PPO; the
 * expert drives env e this step iff u01(seed, call, env_id0 + e, 16, 0) < beta (call: steps of this handle so far).  The table is the caller's: table_obs_dev float
 * [pinned_rows + capacity_steps * n_envs][obs_dim], table_act_dev float [..][act_dim]; step slot s, env e is row pinned_rows + s * n_envs + e.  The slot and the call
 * counter live in the handle on the host; the slot wraps.
 *   hrg_dagger_create  checks the descriptor before anything is allocated: HRG_ERR_INVALID for a null argument, a kind that is neither HRG_BC_SAC nor HRG_BC_PPO, n_envs
 *                      < 1, capacity_steps < 1, pinned_rows < 0, a bound that is not finite or act_high[j] <= act_low[j]; HRG_ERR_UNSUPPORTED for obs_dim outside 1 ..
 *                      HRG_OBS_DIM and act_dim outside 1 .. HRG_ACT_DIM.
 *   hrg_dagger_sizes   size_host int64[4] = steps so far (the next call's key), the next slot, the table's valid rows pinned_rows + min(steps, capacity_steps) * n_envs,
 *                      bytes of device memory held.
 *   hrg_dagger_step    one step, asynchronous on `stream`.  view_dev float [n_envs][obs_dim] (copied bit for bit into the table), learner_act_dev float [n_envs][act_dim]
 *                      (SAC: at the policy's scale; PPO: at the env's, not clamped yet), expert_act_dev double [n_envs][HRG_ACT_DIM].  Writes the slot's rows of the table;
 *                      rows_out_dev double [n_envs][HRG_ACT_DIM], what the step kernel reads: c where the expert drives, else low + 0.5 (a + 1) (high - low) in double
 *                      (SAC; four rounded operations, as torch evaluates it) or clamp(a, low, high) in float (PPO), zeros behind act_dim; kept_out_dev float
 *                      [n_envs][act_dim] or NULL: the executed action at the policy's scale (the label, or the learner's own row); and adds to the statistics.  beta
 *                      outside [0, 1] or not finite: HRG_ERR_INVALID.
 *   hrg_dagger_stats   synchronous: per_env_host double [n_envs][HRG_DAGGER_STATS_DIM], the sums since the last clear; `clear` zeroes them on the device. */
int hrg_dagger_create(const hrg_dagger_desc* desc, int32_t device, hrg_dagger** out);
void hrg_dagger_destroy(hrg_dagger* h);
int hrg_dagger_sizes(hrg_dagger* h, int64_t* size_host);
int hrg_dagger_step(hrg_dagger* h, const float* view_dev, const float* learner_act_dev, const double* expert_act_dev, double beta, float* table_obs_dev,
                    float* table_act_dev, double* rows_out_dev, float* kept_out_dev, void* stream);
int hrg_dagger_stats(hrg_dagger* h, double* per_env_host, int32_t clear);

/* Adversarial imitation on the device (csrc/hrgym_disc.h): a discriminator trained to tell a table's (observation, action) rows from the learner's
 * own, and the reward it gives a batch.  The parameters are the caller's float [n_params] device array -- W_l [64][in_l], b_l [64] for l < depth (in_0 = obs_dim +
 * act_dim), W_d [1][64], b_d [1] --, the moments m_dev, v_dev the caller's too, in the same layout, zero at the start.  The handle owns its step count (Adam's, and
 * the key of its draws) and its scratch.
 *   hrg_disc_create   checks the descriptor before anything is allocated: HRG_ERR_INVALID for a null argument, an activation or reward_kind that is none of the
 *                     enumerators; HRG_ERR_UNSUPPORTED for hidden other than HRG_SAC_HIDDEN, depth outside 1 .. 3, obs_dim outside 1 .. HRG_OBS_DIM, act_dim outside
 *                     1 .. HRG_ACT_DIM, a batch_size that is not a multiple of HRG_SAC_TILE in HRG_SAC_TILE .. HRG_DISC_MAX_BATCH.
 *   hrg_disc_sizes    size_host int64[4] = parameters, steps so far, tiles of a step (2 batch_size / HRG_SAC_TILE), batch_size.
 *   hrg_disc_step     one update, two launches, asynchronous on `stream`.  Expert row k < batch_size is the table's row index_in_dev[k] (int64 [batch_size], clamped
 *                     into the table) or, with NULL, floor(u n_rows) clamped to n_rows - 1 with u = u01(seed, step count, k, 17, 0); policy row k is row k of
 *                     policy_obs_dev float [batch_size][obs_dim] and policy_act_dev float [batch_size][act_dim].  The loss is the binary cross-entropy on the logit,
 *                     (1 / 2B) (sum_expert softplus(-d) + sum_policy softplus(d)); then torch's Adam (eps 1e-8).  Only params_dev, m_dev, v_dev and the handle's
 *                     scratch are written.  HRG_ERR_INVALID for a null argument, n_rows < 1, a learning_rate that is not finite or negative.
 *   hrg_disc_reward   forward only, one launch, asynchronous on `stream`: rows obs_dev float [n][obs_dim], act_dev float [n][act_dim], n >= 1.  r_disc = softplus(d)
 *                     (HRG_DISC_REWARD_GAIL) or d (HRG_DISC_REWARD_AIRL) in double; rewards_out_dev float [n] = r_disc, or with env_rewards_dev float [n] (it may be
 *                     rewards_out_dev itself) r_disc alpha + r_env (1 - alpha), rounded once; logits_out_dev float [n] = d.  Either output may be NULL, not both.
 *                     It writes nothing of the discriminator's.  HRG_ERR_INVALID for a null argument, n < 1, alpha outside [0, 1] or not finite.
 *   hrg_disc_export   synchronous parity hook, the last step's: index_host int64 [batch_size] (the table rows), logits_host float [2 batch_size] (expert rows, then
 *                     policy rows), grad_host float [n_params], diag_host float [3] = loss, the share of expert rows with d > 0, of policy rows with d < 0.  Any
 *                     pointer may be NULL.
 *   hrg_disc_restore  sets the step count (a continued run: Adam's bias corrections and the draws' key follow from it). */
int hrg_disc_create(const hrg_disc_desc* desc, int32_t device, hrg_disc** out);
void hrg_disc_destroy(hrg_disc* h);
int hrg_disc_sizes(hrg_disc* h, int64_t* size_host);
int hrg_disc_step(hrg_disc* h, const float* table_obs_dev, const float* table_act_dev, int64_t n_rows, const int64_t* index_in_dev, const float* policy_obs_dev,
                  const float* policy_act_dev, float* params_dev, float* m_dev, float* v_dev, double learning_rate, void* stream);
int hrg_disc_reward(hrg_disc* h, const float* params_dev, const float* obs_dev, const float* act_dev, int32_t n, const float* env_rewards_dev, double alpha,
                    float* rewards_out_dev, float* logits_out_dev, void* stream);
int hrg_disc_export(hrg_disc* h, int64_t* index_host, float* logits_host, float* grad_host, float* diag_host);
int hrg_disc_restore(hrg_disc* h, uint64_t steps);

/* Evaluation on the device (csrc/hrgym_eval.h): SB3 1.5.0's evaluate_policy with deterministic = True as a loop of three launches per env step -- the step entry
 * that fits what is attached, hrg_eval_step, hrg_eval_policy_* -- with no copy to the host between them.  The view float [n_envs][width] and the action rows double
 * [n_envs][HRG_ACT_DIM] are the caller's device arrays, width = n_obs_cols + observe_time, on a goal env ag_dim + dg_dim + n_obs_cols.  All but create / destroy /
 * remaining / export / size are asynchronous on `stream`.  The step counter lives in the handle on the host.
 *   hrg_eval_create      checks the descriptor before anything is allocated: HRG_ERR_INVALID for n_envs < 1, n_policies < 1, n_envs % n_policies != 0,
 *                        n_eval_episodes < 1, a quota ceil(n_eval_episodes / (n_envs / n_policies)) above HRG_EVAL_MAX_EPISODES_PER_ENV, what hrg_replay_create
 *                        refuses of the columns and the statistics, bounds that are not finite or not ordered; HRG_ERR_UNSUPPORTED for goal_env with
 *                        observe_time or normalize, a goal_kind that is no HRG_GOAL_*, a feature row wider than HRG_OBS_DIM.
 *   hrg_eval_begin       after a reset: obs_dev float [n_envs][HRG_OBS_DIM], time_dev float [n_envs] (needed with observe_time) -> every env's running return,
 *                        length and count 0, its quota, view_dev = the policy's view of obs_dev.  The step counter becomes 0.
 *   hrg_eval_step        after a step (the tensors it wrote): the running return adds the env's own reward (column HRG_SIR_R_ENV of sir_dev, HRG_IMIT_R_ENV of
 *                        imit_dev, or reward_dev without either), the running length 1; where done_dev[e] and the env's count is below its quota, record `count`
 *                        of env e is written and the count moves; view_dev = the policy's view of obs_dev (the row after auto-reset) with sir column
 *                        HRG_SIR_TIME_OBS.  imit_dev / sir_dev may be NULL; not both given; sir_dev is needed with observe_time.  Advances the step counter.
 *   hrg_eval_policy_sac  actions_dev = low + 0.5 (tanh(mu) + 1) (high - low) of the actor of parameter set k on the rows of group k, in double, zero behind
 *                        act_dim.  params_dev float [n_policies][n_params] in hrg_sac's layout (`sac` gives the offsets; its obs_dim must be the view's width, its
 *                        act_dim the descriptor's, its device the evaluator's: HRG_ERR_INVALID otherwise).
 *   hrg_eval_policy_ppo  the same with the policy network of hrg_ppo: actions_dev = clamp(mu, low, high).
 *   hrg_eval_remaining   synchronous: remaining_host int64[1] = sum over the envs of quota - count (0: every group has its episodes).
 *   hrg_eval_export      synchronous: counts_host, quota_host int32 [n_envs], records_host double [n_envs][max_quota][HRG_EVAL_RECORD_DIM] (record c of env e is
 *                        valid for c < counts[e]).  Any pointer may be NULL.
 *   hrg_eval_size        size_host int64[4] = max_quota, steps since begin, the view's width, bytes of device memory held. */
int hrg_eval_create(const hrg_eval_desc* desc, int32_t device, hrg_eval** out);
void hrg_eval_destroy(hrg_eval* h);
int hrg_eval_begin(hrg_eval* h, const float* obs_dev, const float* time_dev, float* view_dev, void* stream);
int hrg_eval_step(hrg_eval* h, const float* obs_dev, const float* reward_dev, const uint8_t* done_dev, const int32_t* info_dev, const float* imit_dev,
                  const float* sir_dev, float* view_dev, void* stream);
int hrg_eval_policy_sac(hrg_eval* h, hrg_sac* sac, const float* params_dev, const float* view_dev, double* actions_dev, void* stream);
int hrg_eval_policy_ppo(hrg_eval* h, hrg_ppo* ppo, const float* params_dev, const float* view_dev, double* actions_dev, void* stream);
int hrg_eval_remaining(hrg_eval* h, int64_t* remaining_host, void* stream);
int hrg_eval_export(hrg_eval* h, int32_t* counts_host, int32_t* quota_host, double* records_host);
int hrg_eval_size(hrg_eval* h, int64_t* size_host);

/* Kernel timing hook for bench.py: records HIP events on the launch stream around every step kernel
 * since the last call; returns average kernel milliseconds and the number of launches measured. */
int hrg_batch_kernel_time(hrg_batch* b, double* avg_ms, int64_t* n_launches);

#ifdef __cplusplus
}
#endif
#endif /* HRGYM_H */
