"""Drop-in vectorised / single-env facades over the HIP stepper.

`HipVecEnv` keeps the stable-baselines3 `VecEnv` contract that the reference's training utilities consume
(`make_vec_env(..., vec_env_cls=SubprocVecEnv)`: utils/env_util_SB3.py:75-87, utils/training_utils_SB3.py:60-75):
`reset() -> obs[N,18]`, `step_async(actions)`, `step_wait() -> (obs, rewards, dones, infos)`, auto-reset with
`infos[i]["terminal_observation"]`, Monitor-style `infos[i]["episode"] = {"r","l","t"}`, `TimeLimit.truncated`
(wrappers/time_limit.py:40-43) and the `log_info_keys` of training/config/run/default_training.yaml:18-29.
The wrapper stack of the reference (Monitor -> TimeLimit -> GymWrapper -> ReachHuman) is folded into the batch:
flattening to `[object-state, goal_difference]` (human_reach_ppo_parallel.yaml:14-16) happens in the kernel.

`HipGymEnv` is the single-env gym-0.21 facade (4-tuple step) for config 1 (demos/demo_reach_human_environment.py).

If stable-baselines3 / gym are installed the classes subclass their ABCs; otherwise light stand-ins with the same
attributes are used (neither package is available in the build image).
"""
import os
import time
from collections import OrderedDict

import numpy as np

from ._cstruct import CONST
from .animation import synthetic_clips
from .model import build_model_desc
from .device_path import DevicePath
from .tasks import OBS_KEYS, PICK_PLACE_OBS_KEYS, TASKS, Goal, task_row  # noqa: F401  (the two key lists: names other code imports from here)

try:  # pragma: no cover - not installed in the build image
    from stable_baselines3.common.vec_env import VecEnv as _VecEnvBase
except Exception:  # noqa: BLE001
    class _VecEnvBase:  # minimal stand-in with the attributes SB3 algorithms read
        def __init__(self, num_envs, observation_space, action_space):
            self.num_envs = num_envs
            self.observation_space = observation_space
            self.action_space = action_space

        def step(self, actions):
            self.step_async(actions)
            return self.step_wait()

try:  # pragma: no cover
    from gym import spaces as _spaces
    _Box = _spaces.Box
except Exception:  # noqa: BLE001
    class _Box:
        def __init__(self, low, high, shape=None, dtype=np.float32):
            self.shape = tuple(shape if shape is not None else np.shape(low))
            self.low = np.broadcast_to(np.asarray(low, dtype), self.shape).copy()
            self.high = np.broadcast_to(np.asarray(high, dtype), self.shape).copy()
            self.dtype = np.dtype(dtype)

        def sample(self):
            lo = np.where(np.isfinite(self.low), self.low, -1.0)
            hi = np.where(np.isfinite(self.high), self.high, 1.0)
            return np.random.uniform(lo, hi).astype(self.dtype)

        def contains(self, x):
            x = np.asarray(x)
            return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))

try:  # pragma: no cover
    _DictSpace = _spaces.Dict
except Exception:  # noqa: BLE001
    class _DictSpace:
        def __init__(self, spaces):
            self.spaces = dict(spaces)

        def __getitem__(self, k):
            return self.spaces[k]

INFO_KEYS = [  # column order of the kernel's info block (include/hrgym.h)
    "collision", "collision_type", "n_collisions", "n_collisions_static", "n_collisions_robot", "n_collisions_human",
    "n_collisions_critical", "timeout", "failsafe_interventions", "n_goal_reached", "TimeLimit.truncated", "sim_crash",
    "action_resamples", "n_object_handed_over",
]
_BOOL_KEYS = {"collision", "timeout", "TimeLimit.truncated", "sim_crash"}
_BOOL_ITEMS = [(j, k) for j, k in enumerate(INFO_KEYS) if k in _BOOL_KEYS]
DEFAULT_OBS_KEYS = {env_id: t.obs_keys for env_id, t in TASKS.items()}
# columns of the kernel's observation superset (include/hrgym.h HRG_OBS_DIM) per robosuite observable / modality key
OBS_COLUMNS = {
    "object-state": range(0, 12), "goal_difference": range(12, 18), "robot0_joint_pos": range(18, 24),
    "robot0_joint_vel": range(24, 30), "robot0_eef_pos": range(30, 33), "desired_goal": range(33, 39),
    "robot0_proprio-state": range(18, 33), "goal-state": list(range(33, 39)) + list(range(12, 18)),
    "vec_eef_to_human_lh": range(0, 3), "dist_eef_to_human_lh": range(3, 4), "vec_eef_to_human_rh": range(4, 7),
    "dist_eef_to_human_rh": range(7, 8), "vec_eef_to_human_head": range(8, 11), "dist_eef_to_human_head": range(11, 12),
    # PickPlaceHumanCart (pick_place_human_cartesian_env.py:726-841); zero columns for ReachHuman
    "object_gripped": range(39, 40), "vec_eef_to_object": range(40, 43), "vec_eef_to_target": range(43, 46),
    "gripper_aperture": range(46, 47), "object_pos": range(47, 50), "target_pos": range(50, 53),
    "robot0_gripper_qpos": range(53, 55), "robot0_gripper_qvel": range(55, 57),
    # CollaborativeLiftingCart (collaborative_lifting_cartesian_env.py:982-1085): the board sits in the object columns, its balance in the
    # first target column
    "board_pos": range(47, 50), "vec_eef_to_board": range(40, 43), "board_gripped": range(39, 40), "board_balance": range(50, 51),
    "board_quat": [43, 44, 45, 51],
    "object_quat": range(12, 16),   # the cube tasks: orientation of the manipulation object, (x, y, z, w)
    # the handover tasks' quat_eef_to_object / CollaborativeLiftingCart's quat_eef_to_board, computed like the reference does (see oracle compute_obs_e)
    "quat_eef_to_object": range(57, 61),
    # CollaborativeStackingCart (collaborative_stacking_cartesian_env.py:1306-1524): the vectors to the four cubes (a, b, l, r) take the 12 joint-space columns the cube
    # tasks leave empty; vec_eef_to_object / object_pos follow the cube the robot has to place next; next_target_pos sits in the target columns
    "vec_eef_to_all_objects": list(range(12, 18)) + list(range(33, 39)), "vec_eef_to_object_a": range(12, 15), "vec_eef_to_object_b": range(15, 18),
    "vec_eef_to_object_l": range(33, 36), "vec_eef_to_object_r": range(36, 39), "next_target_pos": range(50, 53),
}


OBS_COLUMNS_TASK = {env_id: t.columns for env_id, t in TASKS.items()}   # per-task column overrides: the same observable name sits in other columns of the superset
for _k in ("hammer_quat", "hammer_gripped", "vec_eef_to_hammer", "vec_eef_to_nail", "hammer_pos", "nail_pos", "nail_hammering_progress", "quat_eef_to_hammer"):
    OBS_COLUMNS.setdefault(_k, OBS_COLUMNS_TASK["CollaborativeHammeringCart"][_k])
OBS_COLUMNS["quat_eef_to_board"] = range(57, 61)   # CollaborativeLiftingCart (hammering overrides it with its constant zeros)


def task_columns(env_id):
    """OBS_COLUMNS as `env_id` fills them."""
    return dict(OBS_COLUMNS, **TASKS[env_id].columns)


# ActionBasedExpertImitationRewardWrapper._add_reward_to_info (action_based_expert_imitation_reward_wrapper.py:107-130): on the infos of done steps
IMITATION_INFO_KEYS = ("ep_im_rew_mean", "ep_env_rew_mean", "ep_full_rew_mean", "im_rew_mean", "env_rew_mean", "full_rew_mean")
# PickPlaceHumanCartStateBasedExpertImitationRewardWrapper._add_reward_to_info (state_based_expert_imitation_reward_wrapper.py:529-540) adds four more
STATE_IMITATION_PP_INFO_KEYS = ("ep_m_im_rew_mean", "ep_g_im_rew_mean", "m_im_rew_mean", "g_im_rew_mean")
# what SB3's rollout loops (and the reference's logging callback, for the imitation keys) look up on every info: stored eagerly where they exist
# (and "task", which a mixed batch stores on every info: reading it must not fill the row)
_EAGER_KEYS = frozenset(("terminal_observation", "episode", "TimeLimit.truncated", "task") + IMITATION_INFO_KEYS + STATE_IMITATION_PP_INFO_KEYS)


class LazyInfo(dict):
    """Per-env info dict whose kernel-derived entries (INFO_KEYS, "action", the expert observations) are filled in on first use.

    SB3's collect loops only `.get()` "episode" / "terminal_observation" / "TimeLimit.truncated" on every info of every step; those
    (with the imitation reward means of done steps and a mixed batch's "task": _EAGER_KEYS) are stored eagerly where they exist, so a 4096-env step does not pay for 4096 x 15 dict entries nobody reads.  Any other access (indexing, `in`,
    iteration, `len`, `==`, `dict(info)`, copy / pickle) materialises the row first; afterwards the object is an ordinary dict."""
    __slots__ = ("_src", "_i")

    def _fill(self):
        src = self._src
        if src is not None:
            self._src = None
            src.fill(self, self._i)

    def get(self, key, default=None):
        if self._src is not None and key not in _EAGER_KEYS:
            self._fill()
        return dict.get(self, key, default)

    def __getitem__(self, key):
        if self._src is not None and key not in _EAGER_KEYS:
            self._fill()
        return dict.__getitem__(self, key)

    def __contains__(self, key):
        if self._src is not None and key not in _EAGER_KEYS:
            self._fill()
        return dict.__contains__(self, key)

    def _filled(name):  # noqa: N805
        def method(self, *a, **k):
            self._fill()
            return getattr(dict, name)(self, *a, **k)
        method.__name__ = name
        return method

    for _n in ("__iter__", "__len__", "__eq__", "__ne__", "__repr__", "__setitem__", "__delitem__", "__or__", "__ror__", "__ior__", "__reversed__",
               "keys", "values", "items", "copy", "pop", "popitem", "setdefault", "update", "clear"):
        locals()[_n] = _filled(_n)
    del _n, _filled
    __hash__ = None

    def __reduce__(self):   # pickle / deepcopy: a plain dict
        self._fill()
        return (dict, (dict(self),))


class _InfoSource:
    """What the infos of one step are filled from: a copy of the info block, the executed actions, the expert views."""

    def __init__(self, rows, acts, expert, prev_full, term_obs, keys=None, early=None):
        self.rows, self.acts, self.expert, self.prev_full, self.term_obs = rows, acts, expert, prev_full, term_obs
        self.keys = keys or INFO_KEYS
        self.early = early   # early_termination per env (state imitation reward with use_et), or None

    def fill(self, d, i):
        row = self.rows[i].tolist()
        set_ = dict.__setitem__
        for k, v in zip(self.keys, row):
            if k != "TimeLimit.truncated":
                set_(d, k, v)
        for j, k in _BOOL_ITEMS:
            if k != "TimeLimit.truncated":
                set_(d, k, row[j] != 0)
        set_(d, "action", self.acts[i])  # collision_prevention_wrapper.py:42-43: the executed action
        if self.early is not None:       # state_based_expert_imitation_reward_wrapper.py:152: on every info when use_et
            set_(d, "early_termination", int(self.early[i]))
        if self.expert is not None:  # expert_obs_wrapper.py:171-175 (the step's own observation: pre-reset where done)
            prev, cur = self.prev_full[i], self.term_obs[i]
            set_(d, "previous_expert_observation", {k: np.array(prev[list(OBS_COLUMNS[k])]) for k in self.expert})
            set_(d, "current_expert_observation", {k: np.array(cur[list(OBS_COLUMNS[k])]) for k in self.expert})


class _TorchBackend:
    """numpy <-> HipBatch / mixed.MixedBatch adapter: one H2D copy of the actions, one D2H copy of the packed output block per step.

    The backend protocol `HipVecEnv` relies on (tests/helpers.OracleBackend is its second implementation):
      required  reset() -> obs [n, HRG_OBS_DIM];  step_async(actions float64 [n, HRG_ACT_DIM]);  step_wait() -> (obs, term_obs, reward, done, info), arrays
                that stay valid until the next step;  executed_actions() -> the action rows as the kernel left them;  close()
      optional  batch (the device batch: state access, collision checks, the dataset collector);  attach_expert(desc) / expert_actions();
                attach_dataset(dataset, rsi_prob, state_imitation_reward, seed);  imit / sir (host rows of the last step, None until attached);
                reset_time (after a dataset reset);  reseed(desc) (for seed(); this backend is rebuilt instead)
    Next to it, what device_path.DevicePath drives: reset_device(), launch_step(rows), reset_time_device(), imitation_rows(); the buffers are that `path`'s."""

    def __init__(self, desc=None, clips=None, n_envs=None, env_id0=0, device=0, batch=None):
        import torch
        from ._lib import HipBatch
        from .dist import packed_views
        self.torch = torch
        self.batch = batch if batch is not None else HipBatch(desc, clips, n_envs, env_id0=env_id0, device=device)
        self.n = self.batch.n
        self._host = torch.empty(self.batch.packed.numel(), dtype=torch.uint8, pin_memory=True)
        v = packed_views(self._host.numpy(), self.n)
        self.obs, self.term_obs, self.reward, self.info, self.done = v["obs"], v["term_obs"], v["reward"], v["info"], v["done"]
        self.imit = None   # host copy of the imitation rows, once an expert with a reward is attached
        self.sir = None    # host copy of the state imitation rows, once a dataset is attached
        self.path = None   # the env's device path (device_path.DevicePath), once the env is built: called after a reset, before and after a step

    def _fetch(self):
        if self.sir is not None:
            self._sir_host.copy_(self.batch.sir, non_blocking=True)
        if self.imit is not None:   # queued ahead of the packed block on the same stream: the one blocking copy below completes both
            self._imit_host.copy_(self.batch.imit, non_blocking=True)
        self._host.copy_(self.batch.packed, non_blocking=False)

    def attach_expert(self, desc):
        self.batch.attach_expert(desc)
        if desc.reward_enabled:
            self._imit_host = self.torch.zeros(self.n, CONST["HRG_IMIT_DIM"], dtype=self.torch.float32, pin_memory=True)
            self.imit = self._imit_host.numpy()

    def attach_dataset(self, dataset, rsi_prob, state_imitation_reward, seed):
        self.batch.attach_dataset(dataset, rsi_prob=rsi_prob, state_imitation_reward=state_imitation_reward, seed=seed)
        self._sir_host = self.torch.zeros(self.n, CONST["HRG_SIR_DIM"], dtype=self.torch.float32, pin_memory=True)
        self.sir = self._sir_host.numpy()

    def expert_actions(self):
        return self.batch.expert_actions().cpu().numpy()

    def reset_device(self):
        """The reset, to a dataset state where a dataset is attached, without the copy to the host (the device loops start here)."""
        if self.sir is not None:
            self.batch.dataset_reset()
            cur = self.batch.dataset_cursor()   # (synchronous; a whole-batch reset is not on the step path)
            self.reset_time = (cur[:, 1] / cur[:, 2]).astype(np.float32)   # StateBasedExpertImitationRewardWrapper.reset (107): start step / T
        else:
            self.batch.reset()

    def reset(self):
        self.reset_device()
        if self.path is not None:
            self.path.after_reset(host=True)
        self._fetch()
        return self.obs

    def launch_step(self, act):
        """The step entry that fits what is attached; `act`: float64 [n, HRG_ACT_DIM] on the device (the kernel may rewrite the rows)."""
        if self.sir is not None:   # (runs the expert's kernels too when an imitation reward is attached)
            self.batch.step_dataset(act)
        elif self.imit is not None:
            self.batch.step_imitation(act)
        else:
            self.batch.step(act)

    def reset_time_device(self):
        """The time values of the rows the last dataset reset left (the state imitation reward's time column): float32 [n] on the device."""
        return self.torch.from_numpy(np.ascontiguousarray(self.reset_time, np.float32)).to(self.batch.device)

    def imitation_rows(self):
        """The last step's imitation rows as the replay buffer and the evaluator take them: dict(sir=...) with a state imitation reward, dict(imit=...) with an
        action imitation reward, else nothing."""
        b = self.batch
        if self.sir is not None and b.dataset_desc.sir_kind != CONST["HRG_SIR_NONE"]:
            return dict(sir=b.sir)
        if self.imit is not None:
            return dict(imit=b.imit)
        return {}

    def step_async(self, actions):
        self._act = self.torch.from_numpy(np.ascontiguousarray(actions, np.float64)).to(self.batch.device, non_blocking=True)
        if self.path is not None:
            self.path.before_step(self._act)
        self.launch_step(self._act)

    def step_wait(self):
        if self.path is not None:
            self.path.after_step()
        self._fetch()
        return self.obs, self.term_obs, self.reward, self.done, self.info

    def executed_actions(self):
        """Actions after CollisionPreventionWrapper screening (the kernel rewrites the action rows in place)."""
        return self._act.cpu().numpy()

    def close(self):
        self.batch.close()


class HipVecEnv(_VecEnvBase):
    """Batched ReachHuman environments stepped by the HIP library (one wavefront per env).

    Args mirror the reference factory (`utils/env_util_SB3.py:19-87`): `env_kwargs` is the dict composed at
    `utils/training_utils.py:71-88`; `seed` plays the role of `seed + rank` (per-env streams are keyed by the
    global env id, so sharding does not change results)."""
    def __init__(self, n_envs=1, env_id="ReachHuman", env_kwargs=None, obs_keys=None, seed=None, clips=None,
                 device=0, env_id0=0, backend=None, info_dicts=True, collision_prevention=None, goal_check=True, ik_position_delta=None,
                 expert_obs_keys=None, goal_env=False, obs_norm=None, monitor_dir=None, monitor_kwargs=None, reach_box=False, robot_geometry="capsule",
                 expert=None, imitation_reward=None, dataset=None, rsi_prob=None, state_imitation_reward=None):
        if env_id not in TASKS:
            raise NotImplementedError(f"env_id {env_id!r}: the HIP stepper covers {sorted(TASKS)} (DESIGN.md §6)")
        self.env_id = env_id
        self._reach_box = bool(reach_box)   # ReachHuman with its free smallBox object (stepped by the cube kernel); default: the lean model
        self._task = task_row(env_id, self._reach_box)
        self._robot_geometry = robot_geometry   # "capsule" (default) | "hull": the arm links collide as the convex hulls of their meshes (every task)
        self._init_dataset(self._check_dataset(dataset, rsi_prob, state_imitation_reward, imitation_reward, backend, goal_env), rsi_prob, state_imitation_reward)
        self._check_expert(expert, imitation_reward, backend, goal_env)
        if goal_env and obs_keys is None:  # goal_env_wrapper.py:62-71
            obs_keys = ["object-state", "robot0_proprio-state", "desired_goal"]
        self._init_columns(obs_keys if obs_keys is not None else self._task.obs_keys, task_columns(env_id), goal_env=goal_env, expert_obs_keys=expert_obs_keys)
        kw = dict(env_kwargs or {})
        if seed is not None:
            kw["seed"] = int(seed)
        self.env_kwargs = kw
        self._clips = clips if clips is not None else synthetic_clips()
        # collision_prevention: dict(replace_type=0|1|2, n_resamples=20) = config/wrappers/collision_prevention/*.yaml
        # ik_position_delta: dict(action_limit=0.15, x_output_max=1, ...) = config/wrappers/ik_position_delta/*.yaml: actions become
        # [dx, dy, dz, gripper] (IKPositionDeltaWrapper, wrappers/ik_position_delta_wrapper.py), converted in the kernel
        self._model_args = dict(collision_prevention=collision_prevention, goal_check=goal_check, env_id=env_id, ik_position_delta=ik_position_delta,
                                reach_box=self._reach_box, robot_geometry=robot_geometry)
        self._desc = self._compose_desc()
        self._device, self._env_id0 = device, env_id0
        self._init_expert(expert, imitation_reward)
        if backend is not None and (isinstance(backend, type) or not hasattr(backend, "step_async")):   # a factory (desc, clips, n_envs, env_id0) -> backend: the caller cannot build the
            backend = backend(self._desc, self._clips, n_envs, env_id0)    # backend itself when the model description is composed here (create_training_vec_env)
        self._backend = backend if backend is not None else self._build_backend(n_envs)
        self._init_spaces(n_envs, collision_prevention, ik_position_delta)
        self._init_accounting(n_envs, info_dicts)
        self.horizon = int(self._desc.horizon)
        self._init_obs_norm(obs_norm)
        self._init_monitor(monitor_dir, monitor_kwargs, n_envs, env_id0)

    # ---- construction, step by step (mixed.MixedHipVecEnv runs the same steps over its own backend) -------------------
    def _check_dataset(self, dataset, rsi_prob, state_imitation_reward, imitation_reward, backend, goal_env):
        """dataset: a name (datasets/<name>/hrg_dataset.npz) or a loaded dataset.ExpertDataset: every episode starts from a state of the dataset
        (DatasetRSIWrapper: a random state with probability rsi_prob, otherwise an episode's first); state_imitation_reward: dict(alpha, beta,
        iota | iota_m, iota_g, sim_fn | m_sim_fn, g_sim_fn, observe_time, use_et, et_dist) = config.wrappers.state_based_expert_imitation_reward:
        the step reward becomes r_im alpha + r_env (1 - alpha), r_im from the demonstration state of the same step (csrc/hrgym_dataset.h).
        Returns the loaded dataset, or None."""
        if dataset is None:
            if rsi_prob is not None or state_imitation_reward is not None:
                raise ValueError("rsi_prob / state_imitation_reward need a dataset (the reference's wrappers load one by dataset_name)")
            return None
        from .dataset import ExpertDataset, check_holds_state
        env_id, has_box = self.env_id, self._task.block == "box"
        if backend is not None:
            raise NotImplementedError("dataset / state_imitation_reward: the restore and reward kernels run in the HIP library; another backend has none")
        if goal_env:
            raise NotImplementedError("dataset / state_imitation_reward with goal_env: the imitation reward is not a function of the goals (no compute_reward)")
        check_holds_state(env_id)
        if state_imitation_reward is not None and imitation_reward is not None:
            raise NotImplementedError("state_imitation_reward with imitation_reward: the reference wraps one imitation reward, state based or action based")
        if not isinstance(dataset, ExpertDataset):
            dataset = ExpertDataset.load(dataset, env_id=env_id, has_box=has_box)
        elif dataset.env_id != env_id or (dataset.boxes is not None) != has_box:
            raise ValueError(f"dataset of {dataset.env_id} ({'with' if dataset.boxes is not None else 'without'} box array) for {env_id}")
        if state_imitation_reward is not None and self._reach_box:
            raise NotImplementedError("state_imitation_reward with reach_box: the cube kernel serves object_quat in the goal_difference columns")
        return dataset

    def _init_dataset(self, dataset=None, rsi_prob=None, state_imitation_reward=None):
        self._dataset = dataset      # the attached demonstration dataset (dataset.ExpertDataset)
        self._sir = None             # arguments of the state imitation reward (dataset.sir_kwargs), when one is configured
        self._observe_time = False   # the state imitation reward appends its time column to the observation
        if dataset is not None:
            self._rsi_prob, self._sir_arg = float(rsi_prob or 0.0), state_imitation_reward
            if state_imitation_reward is not None:
                from .dataset import sir_kwargs
                self._sir = sir_kwargs(self.env_id, state_imitation_reward)
                self._observe_time = self._sir["observe_time"]

    def _check_expert(self, expert, imitation_reward, backend, goal_env):
        """expert: dict(id=..., signal_to_noise_ratio=..., ...) = config.expert (a scripted expert of demonstrations/experts/, evaluated on the device:
        env.expert_actions()); imitation_reward: dict(alpha, beta, iota_m, iota_g, m_sim_fn, g_sim_fn, normalize_joint_actions) =
        config.wrappers.action_based_expert_imitation_reward: the step reward becomes r_im alpha + r_env (1 - alpha) (csrc/hrgym_expert.h)"""
        if imitation_reward is not None and expert is None:
            raise ValueError("imitation_reward needs an expert (the reference asserts: No expert specified in config!)")
        if expert is None:
            return
        from .expert import EXPERT_ENVS, expert_kwargs
        if backend is not None:
            raise NotImplementedError("expert / imitation_reward: the experts run in the HIP library; another backend has none")
        if goal_env:
            raise NotImplementedError("expert / imitation_reward with goal_env: the imitation reward is not a function of the goals (no compute_reward)")
        eid, _ = expert_kwargs(expert)
        if eid not in self._task.experts:
            raise NotImplementedError(f"expert {eid}: it reads the observation of {EXPERT_ENVS[eid]}, not of {self.env_id}")

    def _init_expert(self, expert=None, imitation_reward=None):
        self._expert_desc = None   # hrg_expert_desc of the attached scripted expert
        self._imit_alpha = None    # alpha of the imitation reward, when one is configured
        if expert is not None:
            from .expert import build_expert_desc
            # the bounds in FP64 as configured (the f32 action space rounds action_limit = 0.1 to 0.100000001)
            hi = [1.0] * CONST["HRG_ACT_DIM"] if self._model_args["ik_position_delta"] is None else [float(self._desc.ik_action_limit)] * 3 + [1.0]
            self._expert_desc = build_expert_desc(expert, [-x for x in hi], hi, imitation_reward, default_seed=int(self._desc.seed))
            if imitation_reward is not None:
                self._imit_alpha = float(self._expert_desc.alpha)

    def _init_columns(self, keys, cols_of, goal_env=False, expert_obs_keys=None):
        """The policy's view of the kernel's observation superset: `keys` concatenated in order (GymWrapper), each looked up in `cols_of`; None: every column."""
        # GoalEnvironmentGymWrapper (wrappers/goal_env_wrapper.py): dict observations {observation, achieved_goal, desired_goal} and an
        # externalised reward for hindsight relabelling.  The goals per task: tasks.Goal
        self.goal_env = bool(goal_env)
        if self.goal_env:
            goal = self._task.goal
            if not isinstance(goal, Goal):
                raise NotImplementedError(f"goal_env: {goal}")
            self._ag_cols, self._dg_cols = np.array(goal.achieved, dtype=np.int64), np.array(goal.desired, dtype=np.int64)
        unknown = [k for k in keys or [] if k not in OBS_COLUMNS and k not in cols_of]   # (a key of OBS_COLUMNS_TASK alone, robot0_eef_velp, exists on its task only)
        if unknown:
            raise NotImplementedError(f"obs_keys {unknown!r}: available {sorted(set(OBS_COLUMNS) | set(cols_of))}")
        self.obs_keys = list(keys) if keys is not None else None
        # ExpertObsWrapper (wrappers/expert_obs_wrapper.py:155-184): infos carry the expert's view of the state before and after the step
        bad = [k for k in (expert_obs_keys or []) if k not in OBS_COLUMNS]
        if bad:
            raise NotImplementedError(f"expert_obs_keys {bad!r}: available {sorted(OBS_COLUMNS)}")
        self.expert_obs_keys = list(expert_obs_keys) if expert_obs_keys is not None else None
        self._expert_cur = None
        self._cols = np.array([c for k in keys for c in cols_of[k]] if keys is not None else range(CONST["HRG_OBS_DIM"]), dtype=np.int64)

    def _compose_desc(self):
        return build_model_desc(self.env_kwargs, n_clips=self._clips.n_clips, **self._model_args)

    def _build_backend(self, n_envs):
        """The HIP batch of `self._desc` with the configured expert and dataset attached (construction, and again after seed())."""
        backend = _TorchBackend(self._desc, self._clips, n_envs, self._env_id0, self._device)
        if self._expert_desc is not None:
            backend.attach_expert(self._expert_desc)
        if self._dataset is not None:
            backend.attach_dataset(self._dataset, self._rsi_prob, self._sir_arg, int(self._desc.seed))
        return backend

    def _init_spaces(self, n_envs, collision_prevention=None, ik_position_delta=None):
        self._cp, self._ik = collision_prevention, ik_position_delta   # the action front-ends: with either, the kernel rewrites the action rows
        obs_space = _Box(-np.inf, np.inf, shape=(len(self._cols),), dtype=np.float32)
        if self._observe_time:   # _add_time_to_observation_space (state_based_expert_imitation_reward_wrapper.py:202-208): one more value, bound to [0, 1]
            obs_space = _Box(np.concatenate([obs_space.low, [0.0]]).astype(np.float32), np.concatenate([obs_space.high, [1.0]]).astype(np.float32), dtype=np.float32)
        if self.goal_env:
            goal_space = _Box(-np.inf, np.inf, shape=(len(self._dg_cols),), dtype=np.float32)
            ag_space = _Box(-np.inf, np.inf, shape=(len(self._ag_cols),), dtype=np.float32)
            obs_space = _DictSpace({"observation": obs_space, "desired_goal": goal_space, "achieved_goal": ag_space})
        if ik_position_delta is None:
            act_space = _Box(-1.0, 1.0, shape=(CONST["HRG_ACT_DIM"],), dtype=np.float32)
        else:  # ik_position_delta_wrapper.py:84-88: position delta limits + one gripper dof
            lim = float(self._desc.ik_action_limit)
            act_space = _Box(np.array([-lim] * 3 + [-1.0], np.float32), np.array([lim] * 3 + [1.0], np.float32), dtype=np.float32)
        _VecEnvBase.__init__(self, n_envs, obs_space, act_space)

    def _init_accounting(self, n_envs, info_dicts):
        self.info_dicts = info_dicts
        self._info_keys = [dict(self._task.info_aliases).get(k, k) for k in INFO_KEYS] if self.env_id in TASKS else list(INFO_KEYS)   # names of the info columns (a task may rename its task-specific one; a mixed batch does not)
        self._ep_ret = np.zeros(n_envs, np.float64)
        self._ep_len = np.zeros(n_envs, np.int64)
        self._t_start = time.time()
        self._actions = None
        self._last_full = None
        self._device_path = DevicePath(self)   # the buffers, learners and loops beside the stepper; survives seed()

    def _init_obs_norm(self, obs_norm=None):
        """DatasetObsNormWrapper (wrappers/dataset_wrapper.py:160-300): (obs - mean) / std, optionally tanh(squash_factor * .), applied to the policy's
        flat observation (and to terminal observations); std == 0 -> 1; shorter / longer statistics are padded / cut when allowed (223-239)"""
        self._norm = None   # (mean, std, squash_factor), when configured
        if obs_norm is None:
            return
        if self.goal_env:
            raise NotImplementedError("obs_norm with goal_env: the reference normalises flat observations only")
        mean, std = np.array(obs_norm["mean"], np.float64), np.array(obs_norm["std"], np.float64)
        k = len(self._cols) + int(self._observe_time)   # the time column is appended inside the normalisation (the imitation wrapper sits below it)
        if mean.shape != (k,) or std.shape != (k,):
            if not obs_norm.get("allow_different_observation_shapes", False):
                raise ValueError(f"obs_norm: statistics of length {mean.shape[0]} for an observation of length {k} (Environment and dataset observation space do not match!)")
            mean = np.concatenate([mean, np.zeros(max(0, k - len(mean)))])[:k]
            std = np.concatenate([std, np.ones(max(0, k - len(std)))])[:k]
        std[std == 0] = 1
        self._norm = (mean, std, obs_norm.get("squash_factor"))
        if self._norm[2] is not None:
            self.observation_space = _Box(-1.0, 1.0, shape=(k,), dtype=np.float32)

    def _init_monitor(self, monitor_dir=None, monitor_kwargs=None, n_envs=None, env_id0=0):
        """Monitor (SB3 [UPSTREAM]; utils/env_util_SB3.py:60-66 gives every worker <monitor_dir>/<rank>.monitor.csv): ONE csv for the batch, same header and
        r,l,t rows (+ info_keywords columns), which stable_baselines3.common.monitor.load_results() reads like any other *.monitor.csv"""
        self._monitor, self._monitor_keys = None, ()   # the open csv, when monitor_dir is given
        if monitor_dir is None:
            return
        import json
        os.makedirs(monitor_dir, exist_ok=True)
        self._monitor_keys = tuple((monitor_kwargs or {}).get("info_keywords", ()))
        path = os.path.join(monitor_dir, f"hip_batch_{int(env_id0)}.monitor.csv")
        self._monitor = open(path, "w", newline="")
        self._monitor.write("#" + json.dumps({"t_start": self._t_start, "env_id": self.env_id, "n_envs": int(n_envs)}) + "\n")
        self._monitor.write(",".join(("r", "l", "t") + self._monitor_keys) + "\n")
        self._monitor.flush()

    # ---- VecEnv API -------------------------------------------------------------------------------------
    def reset(self):
        self._ep_ret[:] = 0
        self._ep_len[:] = 0
        full = np.asarray(self._backend.reset())
        self._last_full = full
        if self.expert_obs_keys is not None:
            self._expert_cur = np.array(full, copy=True)
        return self._view(full, self._backend.reset_time if self._observe_time else None)

    def step_async(self, actions):
        if self._device_path.loop:
            raise RuntimeError(f"step_async after {self._device_path.loop}: the device loop moved the envs on without the host accounting (episode returns, the last "
                               "observation); call reset() first")
        if self._ik is not None:  # [dx, dy, dz, gripper] in the first four columns of the 7-wide action rows
            a4 = np.asarray(actions, np.float64).reshape(self.num_envs, 4)
            actions = np.zeros((self.num_envs, CONST["HRG_ACT_DIM"]))
            actions[:, :4] = a4
        actions = np.asarray(actions, np.float64).reshape(self.num_envs, CONST["HRG_ACT_DIM"])
        self._actions = actions
        self._backend.step_async(actions)

    def step_wait(self):
        obs, term_obs, reward, done, info = self._backend.step_wait()
        full = np.asarray(obs)
        self._last_full = full
        sir = np.array(self._backend.sir, copy=True) if self._dataset is not None else None
        obs, reward = self._view(full, sir[:, CONST["HRG_SIR_TIME_OBS"]] if self._observe_time else None), np.array(reward, copy=True)
        dones = np.asarray(done).astype(bool)   # (with early termination: where the episode ended for either reason)
        imit = None
        if self._sir is not None:   # as below: Monitor sits inside the imitation wrapper, its return is r_env (it does not see ET in the reference; here an
            self._ep_ret += sir[:, CONST["HRG_SIR_R_ENV"]]   # ET step ends the Monitor episode like any other done: DESIGN.md deviations)
        elif self._imit_alpha is not None:   # the reward is the combined one; Monitor sits inside the imitation wrapper (SB3 make_vec_env), so its return is r_env
            imit = np.array(self._backend.imit, copy=True)
            self._ep_ret += imit[:, 1]
        else:
            self._ep_ret += reward
        self._ep_len += 1
        if (self._cp is not None or self._ik is not None) and self.info_dicts:
            self._actions = np.array(self._backend.executed_actions(), copy=True)
        if self.info_dicts:
            infos = self._make_infos(info, dones, term_obs, sir)
            if imit is not None:
                self._imitation_infos(infos, imit, np.nonzero(dones)[0])
            if self._sir is not None:
                self._state_imitation_infos(infos, sir, np.nonzero(dones)[0])
        else:
            infos = [{} for _ in range(self.num_envs)]
            if self._monitor is not None:   # the Monitor csv does not depend on the per-env dicts: episode rows from the done mask and the info block
                self._monitor_rows(np.asarray(info), np.nonzero(dones)[0])
        if self.expert_obs_keys is not None:
            self._expert_cur = np.array(full, copy=True)   # after an auto-reset: the new episode's first observation (wrapper reset())
        self._ep_ret[dones] = 0
        self._ep_len[dones] = 0
        return obs, reward, dones, infos

    def _make_infos(self, info, dones, term_obs, sir=None):
        # the per-env dicts are filled from a copy of the info block on first use (LazyInfo); `sir`: the step's state imitation rows, with a dataset
        info = np.array(info, copy=True)
        src = _InfoSource(info, self._actions, self.expert_obs_keys, self._expert_cur, np.array(term_obs, copy=True) if self.expert_obs_keys is not None else None,
                          keys=self._info_keys, early=sir[:, CONST["HRG_SIR_EARLY"]] if self._sir is not None and self._sir["use_et"] else None)
        n = self.num_envs
        new = LazyInfo.__new__
        infos = [new(LazyInfo) for _ in range(n)]
        for i, d in enumerate(infos):
            d._src = src
            d._i = i
        idx = np.nonzero(dones)[0]
        if len(idx):
            now = round(time.time() - self._t_start, 6)
            trunc = info[idx, INFO_KEYS.index("TimeLimit.truncated")] != 0
            set_ = dict.__setitem__
            for i, tr in zip(idx.tolist(), trunc.tolist()):
                d = infos[i]
                set_(d, "TimeLimit.truncated", tr)
                set_(d, "terminal_observation", self._view(np.array(term_obs[i]), sir[i, CONST["HRG_SIR_TIME"]] if self._observe_time else None))
                set_(d, "episode", {"r": float(self._ep_ret[i]), "l": int(self._ep_len[i]), "t": now})
            if self._monitor is not None:
                self._monitor_rows(info, idx, now)
        return infos

    @staticmethod
    def _reward_means(d, ep_im, ep_env, n, a):
        """The six entries both _add_reward_to_info write on the info of a done step: episode sums and per-step means of r_im, r_env and their mix by alpha."""
        set_ = dict.__setitem__
        set_(d, "ep_im_rew_mean", ep_im)
        set_(d, "ep_env_rew_mean", ep_env)
        set_(d, "ep_full_rew_mean", ep_im * a + ep_env * (1 - a))
        set_(d, "im_rew_mean", ep_im / n)
        set_(d, "env_rew_mean", ep_env / n)
        set_(d, "full_rew_mean", (ep_im / n) * a + (ep_env / n) * (1 - a))

    def _imitation_infos(self, infos, imit, idx):
        """_add_reward_to_info (action_based_expert_imitation_reward_wrapper.py:107-130) from the imitation rows of the envs that finished an episode."""
        for i in idx.tolist():
            self._reward_means(infos[i], float(imit[i, 4]), float(imit[i, 5]), float(imit[i, 6]), self._imit_alpha)

    def _state_imitation_infos(self, infos, sir, idx):
        """_add_reward_to_info of the state-based wrappers (state_based_expert_imitation_reward_wrapper.py:176-200, 529-540) from the rows of the envs that
        finished an episode; the pick-place means divide by the steps that entered the motion / gripper sums (535)."""
        C = CONST
        pp = self._backend.batch.dataset_desc.sir_kind == C["HRG_SIR_PICK_PLACE"]
        set_ = dict.__setitem__
        for i in idx.tolist():
            row, d = sir[i], infos[i]
            self._reward_means(d, float(row[C["HRG_SIR_EP_IM"]]), float(row[C["HRG_SIR_EP_ENV"]]), float(row[C["HRG_SIR_EP_LEN"]]), self._sir["alpha"])
            if pp:
                ep_m, ep_g, n_mg = float(row[C["HRG_SIR_EP_MOTION"]]), float(row[C["HRG_SIR_EP_GRIPPER"]]), float(row[C["HRG_SIR_EP_LEN_MG"]])
                set_(d, "ep_m_im_rew_mean", ep_m)
                set_(d, "ep_g_im_rew_mean", ep_g)
                set_(d, "m_im_rew_mean", float("nan") if n_mg == 0 else ep_m / n_mg)
                set_(d, "g_im_rew_mean", float("nan") if n_mg == 0 else ep_g / n_mg)

    def expert_actions(self):
        """The attached expert's action for every env's current observation (the one the last reset / step returned): float64 [n, 4] for the
        Cartesian experts, [n, 7] for ReachHuman's.  Every call advances the expert's noise process once, like a call of the reference's expert."""
        if self._expert_desc is None:
            raise NotImplementedError("expert_actions: construct the env with expert=dict(id=..., ...)")
        if self._last_full is None:
            raise RuntimeError("expert_actions: call reset() first")
        a = np.asarray(self._backend.expert_actions(), np.float64)
        return np.array(a[:, :4] if self._expert_desc.cartesian else a, copy=True)

    def _monitor_rows(self, info, idx, now=None):
        """One r,l,t(+info_keywords) row per finished episode (SB3 Monitor [UPSTREAM]); info_keywords are columns of the kernel's info block."""
        if not len(idx):
            return
        now = round(time.time() - self._t_start, 6) if now is None else now
        for i in idx.tolist():
            extra = []
            keys = list(self._info_keys)
            for k in self._monitor_keys:
                if k not in keys:
                    raise KeyError(f"Monitor info_keywords: {k!r} is not a column of the info block ({keys})")
                v = int(info[i, keys.index(k)])
                extra.append(str(bool(v)) if k in _BOOL_KEYS else str(v))
            self._monitor.write(",".join([f"{round(float(self._ep_ret[i]), 6)}", str(int(self._ep_len[i])), str(now)] + extra) + "\n")
        self._monitor.flush()

    def close(self):
        if self._monitor is not None:
            self._monitor.close()
            self._monitor = None
        self._device_path.close()
        self._backend.close()

    def seed(self, seed=None):
        """Re-key the per-env random streams (takes effect at the next reset by rebuilding the batch)."""
        if seed is None:
            return [None] * self.num_envs
        self.env_kwargs["seed"] = int(seed)
        self._desc = self._compose_desc()
        if isinstance(self._backend, _TorchBackend):
            self._device_path.close_buffers()
            self._backend.close()
            self._backend = self._build_backend(self.num_envs)
            self._device_path.rebind()   # (every attached buffer anew, empty)
        else:
            self._backend.reseed(self._desc)
        return [int(seed) + i for i in range(self.num_envs)]

    def get_attr(self, attr_name, indices=None):
        idx = self._indices(indices)
        if attr_name in ("horizon", "env_kwargs"):
            return [getattr(self, attr_name)] * len(idx)
        if attr_name == "joint_pos":   # env.robots[0].controller.joint_pos (ik_position_delta_wrapper.py:107): the arm's joint angles after the last step / reset
            if self._last_full is None:
                raise RuntimeError("joint_pos: call reset() first")
            return [np.array(self._last_full[i, 18:24], np.float64) for i in idx]
        raise AttributeError(f"HipVecEnv has no per-env attribute {attr_name!r}")

    # HumanEnv.get_environment_state / set_environment_state (human_env.py:1845-1900; used by the dataset / reference-state-initialisation wrappers):
    # the stepper's state blocks, batched.  Each entry is (hrg_env_state, hrg_box_state or None); a restored episode keeps its own random streams.
    def _hip_batch(self, method, what):
        batch = getattr(self._backend, "batch", None)
        if batch is None or not hasattr(batch, method):
            raise NotImplementedError(f"{what} needs the HIP batch backend")
        return batch

    def get_environment_state(self, indices=None):
        batch = self._hip_batch("get_states", "get_environment_state")
        idx = self._indices(indices)
        states, boxes = batch.get_states(np.asarray(idx, np.int32))
        block = self._task.block
        if block in ("stack", "hammer"):   # CollaborativeStackingEnvState / CollaborativeHammeringEnvState: the task's own block next to the state
            get = batch.get_stack if block == "stack" else batch.get_hammer
            return [(st, get(i)) for st, i in zip(states, idx)]
        return [(st, boxes[k] if block == "box" else None) for k, st in enumerate(states)]

    def set_environment_state(self, states, indices=None):
        batch = self._hip_batch("set_states", "set_environment_state")
        idx = self._indices(indices)
        if len(states) != len(idx):
            raise ValueError(f"{len(states)} states for {len(idx)} envs")
        from ._cstruct import BoxState, EnvState
        st_arr = (EnvState * len(idx))(*[st for st, _ in states])
        block = self._task.block
        if block in ("stack", "hammer"):
            batch.set_states(np.asarray(idx, np.int32), st_arr, None)
            for i, (_, sk) in zip(idx, states):
                (batch.set_stack if block == "stack" else batch.set_hammer)(i, sk)
            return
        boxes = [b for _, b in states]
        bx_arr = (BoxState * len(idx))(*boxes) if all(b is not None for b in boxes) and block == "box" else None
        batch.set_states(np.asarray(idx, np.int32), st_arr, bx_arr)

    def check_collision_action(self, actions):
        """HumanEnv.check_collision_action (human_env.py:588-627) for every env: bool array, True where the joint-space action would drive the robot
        into the static scene or itself.  Nothing is stepped."""
        batch = self._hip_batch("check_actions", "check_collision_action")
        a = np.asarray(actions, np.float64).reshape(self.num_envs, CONST["HRG_ACT_DIM"])
        import torch
        return batch.check_actions(torch.from_numpy(np.ascontiguousarray(a))).cpu().numpy().astype(bool)

    def set_attr(self, attr_name, value, indices=None):
        raise NotImplementedError("per-env attributes are fixed at construction (hrg_model_desc)")

    def _view(self, full, time=None):
        """Policy view of rows of the observation superset: flat array, or the goal-env dict.  `time`: the state imitation reward's time column (observe_time)."""
        full = np.asarray(full)
        if not self.goal_env:
            v = full[..., self._cols]
            if time is not None:
                v = np.concatenate([v, np.asarray(time, np.float32)[..., None]], axis=-1)
            if self._norm is not None:
                mean, std, squash = self._norm
                v = (v - mean) / std
                if squash is not None:
                    v = np.tanh(squash * v)
                v = v.astype(np.float32)
            return v
        return {"observation": full[..., self._cols], "achieved_goal": full[..., self._ag_cols], "desired_goal": full[..., self._dg_cols]}

    def compute_reward(self, achieved_goal, desired_goal, info):
        """GoalEnvironmentGymWrapper.compute_reward -> HumanEnv._compute_reward (human_env.py:629-664, 766-792), vectorised: sparse task
        reward (+ 1 + dense reward when shaping), collision penalty from info["collision_type"], reward scale.  `info` is one dict or a
        sequence of dicts (as SB3's HerReplayBuffer passes them)."""
        if not self.goal_env:
            raise NotImplementedError("compute_reward: construct with goal_env=True / make_vec_env(type='goal_env')")
        d = self._desc
        ag, dg = np.atleast_2d(np.asarray(achieved_goal, np.float64)), np.atleast_2d(np.asarray(desired_goal, np.float64))
        infos = [info] if isinstance(info, dict) else list(info)
        ctype = np.array([int(i.get("collision_type", 0)) for i in infos])
        if self._task.goal.rule == "distance":   # joint angles / eef positions: the Euclidean distance of the goals
            dist = np.linalg.norm(ag - dg, axis=-1)
            r = np.where(dist <= d.goal_dist, d.task_reward, -1.0)
            dense = -0.1 * dist
        else:
            e2o, o2t = np.linalg.norm(ag[:, 3:6] - ag[:, 0:3], axis=-1), np.linalg.norm(dg - ag[:, 3:6], axis=-1)
            r = np.where(o2t <= d.goal_dist, d.task_reward, np.where(ag[:, 6] != 0, d.object_gripped_reward, -1.0))
            dense = -(e2o * 0.2 + o2t) * 0.1
        if d.reward_shaping:
            r = r + 1.0 + dense
        illegal = (ctype & (CONST["HRG_COL_STATIC"] | CONST["HRG_COL_ROBOT"] | CONST["HRG_COL_HUMAN_CRIT"])) != 0
        r = (r + np.where(illegal, d.collision_reward, 0.0)) * d.reward_scale
        return float(r[0]) if isinstance(info, dict) and np.ndim(achieved_goal) == 1 else r.astype(np.float32)

    def compute_done(self, achieved_goal, desired_goal, info):
        """HumanEnv._check_done (human_env.py:835-858), vectorised, in the calling forms of `compute_reward`: (done_at_collision and an illegal collision in
        info["collision_type"]) or (done_at_success and success); success is ||achieved - desired|| <= goal_dist (reach_human_env.py:457-475), for the
        cube tasks ||desired - object_pos|| <= goal_dist (pick_place_human_cartesian_env.py:528-548).  What the patched HerReplayBuffer asks for every
        relabelled transition (wrappers/HER_buffer_add_monkey_patch.py:234-246)."""
        if not self.goal_env:
            raise NotImplementedError("compute_done: construct with goal_env=True / make_vec_env(type='goal_env')")
        d = self._desc
        ag, dg = np.atleast_2d(np.asarray(achieved_goal, np.float64)), np.atleast_2d(np.asarray(desired_goal, np.float64))
        infos = [info] if isinstance(info, dict) else list(info)
        ctype = np.array([int(i.get("collision_type", 0)) for i in infos])
        dist = np.linalg.norm(ag - dg, axis=-1) if self._task.goal.rule == "distance" else np.linalg.norm(dg - ag[:, 3:6], axis=-1)
        illegal = (ctype & (CONST["HRG_COL_STATIC"] | CONST["HRG_COL_ROBOT"] | CONST["HRG_COL_HUMAN_CRIT"])) != 0
        done = (bool(d.done_at_collision) & illegal) | (bool(d.done_at_success) & (dist <= d.goal_dist))
        return bool(done[0]) if isinstance(info, dict) and np.ndim(achieved_goal) == 1 else done

    def _her_desc(self, n_envs, buffer_size, n_sampled_goal, goal_selection_strategy, relabel_observation, seed):
        """hrg_her_desc of this env: the ring, the sampler, the reward / done rule of `compute_reward` / `compute_done`, the policy's view of a row."""
        from .her import build_her_desc
        cols = [int(c) for c in self._cols]
        dg_in_obs = ()
        if relabel_observation:   # where the `desired_goal` key sits inside `observation`
            keys, at, k0 = self.obs_keys or [], [], 0
            cols_of = task_columns(self.env_id)
            for key in keys:
                if key == "desired_goal":
                    at.append(k0)
                k0 += len(cols_of[key])
            if len(at) != 1:
                raise NotImplementedError("attach_her(relabel_observation=True): obs_keys must list desired_goal exactly once")
            dg_in_obs = range(at[0], at[0] + len(self._dg_cols))
        # custom_add (64-79) stores info["action"] where a wrapper wrote one (CollisionPreventionWrapper, collision_prevention_wrapper.py:43), rescaled to
        # [-1, 1] by the action bounds and clipped; otherwise SB3's buffer_action, which is the policy's action in [-1, 1] already.  IKPositionDeltaWrapper
        # writes none, so behind the IK front-end the buffer keeps the agent's own [dx, dy, dz, gripper] (copied before the step rewrites the row), and
        # since the env receives it at env scale (+-ik_action_limit), the same rescaling brings it back to the policy's scale
        front_end = self._cp is not None or self._ik is not None
        low, high = self.action_space.low, self.action_space.high
        return build_her_desc(n_envs, buffer_size, self.horizon, self._task.goal.kind, cols, act_dim=len(low), model_desc=self._desc,
                              n_sampled_goal=n_sampled_goal, goal_selection_strategy=goal_selection_strategy, seed=int(self._desc.seed) if seed is None else seed,
                              act_low=low if front_end else None, act_high=high if front_end else None, dg_in_obs=dg_in_obs, relabel_observation=relabel_observation)

    def attach_her(self, buffer_size, n_sampled_goal=4, goal_selection_strategy="future", online_sampling=True, relabel_observation=False, seed=None):
        """A hindsight replay buffer on the device (her.HerBuffer; the keywords of SB3's HerReplayBuffer, training/config/algorithm/sac_her.yaml):
        `buffer_size` transitions PER ENV.  From now on reset() and every step put their rows into it without leaving the device, `collect_steps` does the
        same without the host; `env.her.sample(n)` returns device tensors, `env.her.sample_features(n)` the rows `attach_sac`'s learner reads.  Attaching
        again replaces the buffer with an empty one (and, between two runs of the device loop, resets the envs).  Returns the buffer."""
        if not self.goal_env:
            raise NotImplementedError("attach_her: construct with goal_env=True / make_vec_env(type='goal_env')")
        if self._task.goal.kind is None:
            raise NotImplementedError(f"attach_her: the device buffer has no goal kind for {self.env_id} ({self._task.goal.no_kind})")
        if not online_sampling:
            raise NotImplementedError("attach_her(online_sampling=False): offline sampling copies relabelled transitions into a second buffer; the device buffer "
                                      "relabels when it samples")
        if int(buffer_size) <= self.horizon:
            raise ValueError(f"attach_her: buffer_size = {buffer_size} transitions per env cannot hold an episode of horizon {self.horizon} and one more transition")
        if self._cp is not None and self._ik is not None:
            raise NotImplementedError("attach_her: with collision prevention behind the IK front-end the executed action is a joint action, not one of the policy's "
                                      "Cartesian action space")
        self._refuse("attach_her", "her")
        return self._device_path.attach("her", dict(buffer_size=int(buffer_size), n_sampled_goal=int(n_sampled_goal), goal_selection_strategy=goal_selection_strategy,
                                                    relabel_observation=bool(relabel_observation), seed=seed))

    # the attached buffers (attach_her, attach_rollout, attach_replay) and learners (attach_sac, attach_ppo and their populations), or None: device_path.DevicePath holds them
    her, rollout, replay = (property(lambda self, k=k: self._device_path.buffers.get(k)) for k in ("her", "rollout", "replay"))
    sac, sac_population, ppo, ppo_population = (property(lambda self, k=k: self._device_path.learners[k]) for k in ("sac", "sac_population", "ppo", "ppo_population"))

    def device_refusal(self, kind):
        """Why this env cannot carry a device buffer of `kind` ("her" | "rollout" | "replay": its backend, or what it is wrapped in), or None."""
        return self._device_path.refusal(kind)

    def _refuse(self, name, kind):
        why = self.device_refusal(kind)
        if why is not None:
            raise NotImplementedError(f"{name}: {why}")

    # ---- the on-policy device path: SB3's RolloutBuffer and collect_rollouts next to the stepper (rollout.py, csrc/hrgym_rollout.h) ----
    def _rollout_desc(self, n_envs, n_steps, gamma, gae_lambda):
        from .rollout import build_rollout_desc
        return build_rollout_desc(n_envs, n_steps, [int(c) for c in self._cols], act_dim=len(self.action_space.low), gamma=gamma, gae_lambda=gae_lambda)

    def attach_rollout(self, n_steps, gamma=0.99, gae_lambda=0.95):
        """A PPO rollout buffer on the device (rollout.RolloutBuffer; the arguments of SB3's RolloutBuffer, training/config/algorithm/ppo.yaml): `n_steps`
        slots per env.  `collect_rollout` fills it; `env.rollout.get(batch_size)` yields minibatches of device tensors.  Attaching again replaces the
        buffer with an empty one (and, between two rollouts of the device loop, resets the envs).  Collision prevention and the IK front-end run in the step kernel and are accepted.  Returns the buffer."""
        self._refuse("attach_rollout", "rollout")
        return self._device_path.attach("rollout", dict(n_steps=int(n_steps), gamma=float(gamma), gae_lambda=float(gae_lambda)))

    def collect_rollout(self, policy, value_fn):
        """OnPolicyAlgorithm.collect_rollouts on the device: `n_steps` steps of every env into `env.rollout`, then its returns and advantages.
        `policy(obs float32 [n, K]) -> (actions float32 [n, act_dim], values [n], log_probs [n])` and `value_fn(obs) -> values [n]` take and return
        tensors on the env's device.  Per step: the current observation, the policy, the actions clipped to the action bounds and widened to the
        float64 rows the kernel reads, the step, the value of every env's terminal observation (used where the time limit truncated), the slot.  No
        device-to-host copy and no stream synchronisation.  The first call (and the first after reset() or seed()) resets the envs.  Afterwards step_async
        raises until reset(): the host accounting did not see these steps; `env.rollout.episode_stats()` is this path's account of episodes."""
        return self._device_path.collect_rollout(policy, value_fn)

    def attach_ppo(self, **kwargs):
        """The PPO learner on the device next to the rollout buffer (ppo.PpoLearner; its keywords: net_arch, learning_rate, batch_size, n_epochs, clip_range,
        clip_range_vf, normalize_advantage, ent_coef, vf_coef, max_grad_norm, log_std_init, ortho_init, seed).  Needs attach_rollout first: `obs_dim`, `act_dim`
        and the rollout's size are the buffer's, and batch_size must divide n_envs * n_steps.  Returns the learner and keeps it as `env.ppo`:
        `env.collect_rollout(env.ppo.policy, env.ppo.value)`, then `env.ppo.train(env.rollout)`."""
        rb = self.rollout
        if rb is None:
            raise NotImplementedError("attach_ppo: call attach_rollout(n_steps, gamma, gae_lambda) first (the learner takes its observation and action widths from the buffer)")
        from .ppo import PpoLearner
        return self._device_path.attach_learner("ppo", PpoLearner, rb.obs_dim, rb, rollout_size=rb.n * rb.n_steps, seed=kwargs.pop("seed", int(self._desc.seed)), **kwargs)

    def attach_ppo_population(self, n_members, seeds=None, **kwargs):
        """`n_members` PPO learners stepped in the same launches (ppo.PpoPopulation; PpoLearner's keywords but `seed`), after attach_rollout: the envs are
        n_members groups of m = num_envs / n_members consecutive envs, and member p acts in and learns from group p only.  `seeds`: one per member (default:
        the env's seed + p).  learning_rate, clip_range, clip_range_vf, ent_coef, vf_coef and max_grad_norm take a scalar or one value per member (a sweep);
        a sequence for a keyword the members share (batch_size, net_arch, n_epochs, ...) is refused.  Refused before anything is allocated: another backend and the mixed batch, no rollout buffer, envs
        that the members do not divide, a batch_size that does not divide m * n_steps.  Returns the population and keeps it as `env.ppo_population`:
        `env.collect_rollout(pop.policy, pop.value)`, then `pop.train(env.rollout)`; `env.evaluate(pop.p.params, n, learner=pop.member(0))` evaluates the
        members side by side."""
        from .ppo import PpoPopulation, refuse_shared_sequences
        from .rollout import group_rows
        P = self._device_path.members("attach_ppo_population", n_members, seeds, kwargs)
        refuse_shared_sequences(PpoPopulation._shared, kwargs)
        self._refuse("attach_ppo_population", "rollout")
        rb = self.rollout
        if rb is None:
            raise NotImplementedError("attach_ppo_population: call attach_rollout(n_steps, gamma, gae_lambda) first (the members take their observation and action "
                                      "widths from the buffer)")
        try:
            rows = group_rows(rb.n, rb.n_steps, P, kwargs.get("batch_size", 64))[1]
        except NotImplementedError as e:
            raise NotImplementedError(f"attach_ppo_population: {e}") from None
        return self._device_path.attach_learner("ppo_population", PpoPopulation, rb.obs_dim, rb, P, self._device_path.member_seeds(P, seeds), rollout_size=rows, **kwargs)

    # ---- the off-policy device path on flat observations: SB3's ReplayBuffer next to the stepper (replay.py, csrc/hrgym_replay.h) ----
    def _replay_desc(self, n_envs, buffer_size, seed):
        from .replay import build_replay_desc
        mean, std, squash = self._norm if self._norm is not None else (None, None, None)
        return build_replay_desc(n_envs, buffer_size, [int(c) for c in self._cols], act_dim=len(self.action_space.low), observe_time=self._observe_time, mean=mean,
                                 std=std, squash_factor=squash, seed=int(self._desc.seed) if seed is None else seed)

    def attach_replay(self, buffer_size, handle_timeout_termination=True, optimize_memory_usage=False, seed=None):
        """A uniform replay buffer on the device (replay.ReplayBuffer; the keywords of SB3's ReplayBuffer, training/config_icra_2024/.../*-SAC.yaml):
        `buffer_size` transitions IN ALL, max(buffer_size // n_envs, 1) slots of one transition per env.  From now on reset() and every step put their rows
        into it without leaving the device -- as the policy sees them: obs_norm, the time column of a state imitation reward --, `collect_steps` does the same
        without the host; `env.replay.sample(n)` returns device tensors.  The action-based and the state-based imitation reward, a dataset, collision
        prevention and the IK front-end are accepted (the ICRA stack).  Attaching again replaces the buffer with an empty one.  Returns the buffer."""
        self._refuse("attach_replay", "replay")
        if not handle_timeout_termination:
            raise NotImplementedError("attach_replay(handle_timeout_termination=False): the device buffer never hands a timeout out as a termination")
        if optimize_memory_usage:
            raise NotImplementedError("attach_replay(optimize_memory_usage=True): the device buffer keeps observations and next observations apart")
        return self._device_path.attach("replay", dict(buffer_size=int(buffer_size), seed=seed))

    def attach_sac(self, **kwargs):
        """The SAC learner on the device next to its buffer (sac.SacLearner; its keywords: net_arch, learning_rate, gamma, tau, ent_coef, target_entropy,
        batch_size, target_update_interval, seed).  Needs attach_replay first, or on a goal env attach_her: `obs_dim` and `act_dim` are the buffer's -- with
        the hindsight buffer the width of the feature row achieved_goal | desired_goal | observation, which has to fit the kernels' 64 values (select the
        observation's columns with obs_keys).  `policy`: "MlpPolicy" on flat observations, "MultiInputPolicy" on a goal env (the defaults; the other one is
        refused).  Returns the learner and keeps it as `env.sac`: `env.collect_steps(env.sac.act, train_freq)`, then `env.sac.train(env.replay or env.her,
        gradient_steps)`."""
        from .sac import check_policy
        policy = check_policy(kwargs.pop("policy", None), self.goal_env)
        rb = self.her if self.goal_env else self.replay
        if rb is None:
            raise NotImplementedError("attach_sac: call attach_replay(buffer_size) first, or attach_her(buffer_size) on a goal env (the learner takes its observation "
                                      "and action widths from the buffer)")
        obs_dim = rb.obs_dim
        if self.goal_env:
            obs_dim = rb.obs_features
            if obs_dim > CONST["HRG_OBS_DIM"]:
                raise NotImplementedError(f"attach_sac: {policy} would see {rb.ag_dim} + {rb.dg_dim} + {rb.obs_dim} = {obs_dim} values (achieved_goal, desired_goal, "
                                          f"observation); the kernels cover {CONST['HRG_OBS_DIM']}: construct the env with obs_keys that select fewer columns")
        from .sac import SacLearner
        return self._device_path.attach_learner("sac", SacLearner, obs_dim, rb, seed=kwargs.pop("seed", int(self._desc.seed)), **kwargs)

    def attach_sac_population(self, n_members, seeds=None, **kwargs):
        """`n_members` SAC learners stepped in the same launches (sac.SacPopulation; SacLearner's keywords but `seed`), after attach_replay: the envs are
        n_members groups of num_envs / n_members consecutive envs, and member p acts in and learns from group p only.  `seeds`: one per member (default: the
        env's seed + p).  learning_rate, gamma, tau, ent_coef and target_entropy take a scalar or one value per member (a sweep); a sequence for a keyword
        the members share (batch_size, net_arch, target_update_interval) is refused.  Refused: a goal env, envs that the members do not divide, the mixed batch.  Returns the population and
        keeps it as `env.sac_population`: `env.collect_steps(pop.act, train_freq)`, then `pop.train(env.replay, gradient_steps)`."""
        from .sac import SacPopulation
        P = self._device_path.members("attach_sac_population", n_members, seeds, kwargs)
        if self.goal_env:
            raise NotImplementedError("attach_sac_population: goal_env: the hindsight buffer has no grouped sample (populations cover SAC on flat observations)")
        if self.num_envs % P:
            raise NotImplementedError(f"attach_sac_population: num_envs = {self.num_envs} is not divisible by n_members = {P}: every member steps a group of the same size")
        self._refuse("attach_sac_population", "replay")
        rb = self.replay
        if rb is None:
            raise NotImplementedError("attach_sac_population: call attach_replay(buffer_size) first (the members take their observation and action widths from the buffer)")
        return self._device_path.attach_learner("sac_population", SacPopulation, rb.obs_dim, rb, P, self._device_path.member_seeds(P, seeds), **kwargs)

    def collect_steps(self, policy, n_steps):
        """OffPolicyAlgorithm.collect_rollouts on the device: `n_steps` steps of every env (train_freq) into `env.replay`, on a goal env into `env.her`.
        `policy(obs float32 [n, K]) -> actions float32 [n, act_dim]` in [-1, 1] takes and returns tensors on the env's device; on a goal env `obs` is the
        feature row achieved_goal | desired_goal | observation (`env.her.observation()`).  Per step: the current observation, the policy, the actions
        brought to the action bounds (low + 0.5 (a + 1) (high - low)) and widened to the float64 rows the kernel reads, the step with whatever reward kernels
        are attached, the slot (the replay buffer stores the policy's own action, the hindsight buffer what reset() / step() hand it: the rows the step left,
        or behind the IK front-end a copy of the agent's rows).  No device-to-host copy and no stream synchronisation.  The first call (and the first after
        reset() or seed()) resets the envs.  Afterwards step_async raises until reset(): the host accounting did not see these steps;
        `env.replay.episode_stats()` / `env.her.episode_stats()` is this path's account of episodes."""
        return self._device_path.collect_steps(policy, n_steps)

    # ---- behaviour cloning on the device: pre-training an attached learner's actor from a demonstration dataset (bc.py, csrc/hrgym_bc.h) ----
    bc = property(lambda self: self._device_path.bc, doc="the attached behaviour cloning (attach_bc), or None")

    def demonstrations(self, dataset, algorithm=None):
        """The (observation, expert action) pairs of a demonstration dataset as a device table (bc.DemoTable) for `attach_bc`.  `dataset`: a name
        (datasets/<name>/hrg_dataset.npz), a path or a dataset.ExpertDataset.  Observations: every episode's rows 0 .. T_k - 1 (the terminal row has no
        action), with a time column the value t / T_k, passed through the attached buffer's own view -- exactly what collect_steps / collect_rollout will show
        the policy.  Actions: the first act_dim columns, clipped to the action bounds; with the replay buffer attached (SAC) rescaled to [-1, 1] by the bounds,
        the scale the buffer stores; with the rollout buffer (PPO) left at the env's scale, which PpoLearner.policy emits.  `algorithm` "sac" | "ppo": which of
        the two, where both buffers are attached.  ValueError for a dataset of another task, of the other action form (cartesian) or of the other arm geometry
        (robot_geometry); NotImplementedError without an attached buffer, on a goal env and on the mixed batch."""
        return self._device_path.demonstrations(dataset, algorithm)

    def attach_bc(self, table, batch_size=128, learning_rate=1e-3, seed=None):
        """Behaviour cloning of the attached lone learner's actor on `table` (env.demonstrations(dataset)): bc.BehaviourCloning, kept as `env.bc`.  Call it
        after attach_sac / attach_ppo; a population is refused.  `bc.train(n)` runs n steps of two launches each, nothing synchronises; it writes into
        `learner.p.params` in place -- the actor's hidden layers and mean head only; the learner's optimiser state, counters and every other parameter stay
        bit for bit -- so that learner.act / learner.policy, evaluate, learner.save and learner.train go on as before.  `seed` (of the index draws): default the
        env's."""
        return self._device_path.attach_bc(table, batch_size=batch_size, learning_rate=learning_rate, seed=seed)

    # ---- DAgger on the device: the learner's own states, labelled by the live scripted expert (dagger.py, csrc/hrgym_dagger.h) ----
    dagger = property(lambda self: self._device_path.dagger, doc="the attached DAgger step and its table (attach_dagger), or None")

    def attach_dagger(self, capacity, beta=0.5, table=None, seed=None):
        """The DAgger step for the attached lone learner and the table it fills (dagger.Dagger, kept as `env.dagger`; `env.dagger.table` is what
        `env.attach_bc` takes).  Call it after attach_sac (with attach_replay) or attach_ppo (with attach_rollout), on an env constructed with expert=....
        `capacity`: transitions in all, like attach_replay's buffer_size: max(capacity // num_envs, 1) step slots of one row per env, the oldest step
        overwritten.  `beta`: the probability that the expert drives an env's step, drawn per env and step (`env.dagger.beta` may be scheduled).  `table`: a
        bc.DemoTable of `env.demonstrations(...)`, copied into the head of the table and never overwritten (DAgger's iteration 0); without one the table is
        empty until the first step.  `seed` (of the mixing draws): default the env's.  Attaching again replaces the handle and its table; seed() rebuilds them
        empty; close() frees them.  NotImplementedError, before anything is allocated: no expert; an imitation_reward (the step's own expert call would advance
        the expert's noise a second time: label and reward would see different expert actions); no lone learner, or a population; a goal env; the mixed
        batch; another backend.
        Every collect_dagger step calls the expert once, which advances its Ornstein-Uhlenbeck noise once: clean labels need the expert's
        signal_to_noise_ratio = 1."""
        return self._device_path.attach_dagger(capacity, beta, table, seed)

    def collect_dagger(self, n_steps, deterministic=True):
        """`n_steps` steps of every env driven by the mixture of the attached learner and the scripted expert, every visited row labelled by the expert and
        written into `env.dagger.table`.  Per step: the attached buffer's view of the current rows, the learner's action (`env.sac.act(obs, deterministic)` or
        `env.ppo.policy(obs, deterministic)[0]`), the expert's action for the same rows, the dagger step (label, per-env draw of who drives, the table's rows,
        the rows the kernel reads), the env step with whatever reward kernels are attached, and with a replay buffer the slot: the executed action at the
        policy's scale, so that with beta = 1 the buffer fills with the expert's transitions, rewards included.  The rollout buffer is not filled (a mixture
        policy is not on-policy); its current rows follow the envs, and the next collect_rollout starts from a reset.  No device-to-host copy and no stream
        synchronisation.  With beta = 0 the envs execute bit for bit the rows collect_steps(learner.act) sends.  The first call (and the first after reset() or
        seed()) resets the envs; afterwards step_async raises until reset(); `env.dagger.stats()` is this loop's account: steps, the share the expert drove, the
        on-policy imitation error.  A Monitor csv is refused.
        Every step advances the expert's Ornstein-Uhlenbeck noise once; clean labels need the expert's signal_to_noise_ratio = 1.  Returns env.dagger."""
        return self._device_path.collect_dagger(n_steps, deterministic)

    # ---- adversarial imitation on the device: a discriminator's reward for SAC (adversarial.py, csrc/hrgym_disc.h) ----
    discriminator = property(lambda self: self._device_path.discriminator, doc="the attached discriminator (attach_discriminator), or None")

    def attach_discriminator(self, table, net_arch=(64, 64), activation="relu", batch_size=128, learning_rate=3e-4, reward="gail", seed=None):
        """The discriminator of adversarial imitation (adversarial.Discriminator, kept as `env.discriminator`): a network on (observation, action) rows trained
        to tell the rows of `table` from the learner's own, whose output `adversarial.train_sac(learner, env.replay, env.discriminator, n, alpha=...)` mixes
        into SAC's reward at sample time, r_disc alpha + r_env (1 - alpha).  `table`: a bc.DemoTable of `env.demonstrations(...)` or a dagger.DaggerTable, of
        kind "sac" (a "ppo" table holds its actions at the env's scale: ValueError); or a dataset name, path or dataset.ExpertDataset, which goes through
        `env.demonstrations` first, with its refusals.  `reward`: "gail" (-log(1 - D)) or "airl" (logit D).  `batch_size`: the learner's.  `seed` (of the
        index draws and the initial weights): default the env's.  Attaching again replaces the handle; seed() leaves it alone, as it leaves the learners;
        close() frees it.  NotImplementedError, before anything is allocated: a goal env, the mixed batch, another backend."""
        return self._device_path.attach_discriminator(table, net_arch=net_arch, activation=activation, batch_size=batch_size, learning_rate=learning_rate, reward=reward,
                                                      seed=seed)

    # ---- evaluation on the device: SB3's evaluate_policy next to the stepper (evaluation.py, csrc/hrgym_eval.h) ----
    def _eval_desc(self, n_envs, n_policies, n_eval_episodes):
        """hrg_eval_desc of this env: the groups and their quotas, the policy's view of a row (obs_keys, obs_norm, the time column; on a goal env the feature
        row), the action bounds."""
        from .evaluation import build_eval_desc
        if self.goal_env and self._task.goal.kind is None:
            raise NotImplementedError(f"evaluate on a {self.env_id} goal env: the device feature row has no goal kind for this task (as attach_her)")
        mean, std, squash = self._norm if self._norm is not None else (None, None, None)
        return build_eval_desc(n_envs, n_policies, n_eval_episodes, [int(c) for c in self._cols], self.action_space.low, self.action_space.high,
                               observe_time=self._observe_time, mean=mean, std=std, squash_factor=squash,
                               goal_kind=self._task.goal.kind if self.goal_env else None)

    def evaluate(self, learner_or_params, n_eval_episodes=10, sync_every=16, learner=None, deterministic=True, render=False):
        """SB3's evaluate_policy(deterministic=True) on the device: `n_eval_episodes` episodes of the deterministic policy, three launches per env step (the
        step, the episode ledger, the fused actor) and no torch op or host copy between them.  `learner_or_params`: a sac.SacLearner / ppo.PpoLearner, or a
        stacked float32 [P, n_params] tensor of parameter sets together with `learner`, whose shapes they follow: the batch is then P groups of num_envs / P
        consecutive envs, group k stepped by row k, `n_eval_episodes` each.  Needs no attached buffer: the view is the env's own (obs_keys, obs_norm, the time
        column of a state imitation reward, the feature row of a goal env).  The envs are reset first; afterwards step_async raises until reset().  Attached
        buffers see none of the evaluation's steps (an open episode of theirs is dropped by the reset), and the next collect_steps / collect_rollout resets the
        envs again, so that its transitions start from rows the buffers hold.  At most
        max quota x horizon + `sync_every` steps (TimeLimit ends every episode); every `sync_every` steps one integer is read back.  Returns an
        evaluation.EvalResult; the returns are the env's own reward, also under an imitation reward."""
        if not deterministic:
            raise NotImplementedError("evaluate(deterministic=False): the device loop runs the deterministic actor (the reference evaluates with deterministic=True)")
        if render:
            raise NotImplementedError("evaluate(render=True): the batched envs have no renderer")
        if not isinstance(self._backend, _TorchBackend):
            raise NotImplementedError("evaluate: the ledger and actor kernels run in the HIP library; another backend (the mixed batch included) has none")
        params = None
        if not hasattr(learner_or_params, "p"):
            params = learner_or_params
            if learner is None:
                raise ValueError("evaluate: a stacked parameter tensor comes with learner=..., whose shapes it follows")
            if params.dim() != 2 or int(params.shape[1]) != learner.p.n_params:
                raise ValueError(f"evaluate: expected parameters [P, {learner.p.n_params}], got {tuple(params.shape)}")
        else:
            learner = learner_or_params
        if getattr(learner, "_prefix", None) not in ("hrg_sac", "hrg_ppo"):
            raise NotImplementedError(f"evaluate: {type(learner).__name__}: the fused actor covers sac.SacLearner and ppo.PpoLearner (an SB3 model is stepped on the host)")
        sync_every = int(sync_every)
        if sync_every < 1:
            raise ValueError(f"evaluate: sync_every = {sync_every} must be positive")
        return self._device_path.evaluate(learner, params, n_eval_episodes, sync_every)

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        if method_name == "check_collision_action":   # per-env call of the reference: env_method("check_collision_action", action, indices=[i])
            idx = self._indices(indices)
            acts = np.zeros((self.num_envs, CONST["HRG_ACT_DIM"]))
            acts[idx] = np.asarray(method_args[0], np.float64)
            return [bool(x) for x in self.check_collision_action(acts)[idx]]
        if method_name == "compute_reward":   # SB3 HerReplayBuffer: env_method("compute_reward", achieved, desired, infos, indices=[0])
            return [self.compute_reward(*method_args, **method_kwargs) for _ in self._indices(indices)]
        if method_name == "compute_done":     # the reference's patched buffer: env_method("compute_done", next_achieved, desired, infos)
            return [self.compute_done(*method_args, **method_kwargs) for _ in self._indices(indices)]
        raise NotImplementedError(f"env_method({method_name!r}) is not available on the batched stepper")

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * len(self._indices(indices))

    def get_images(self):
        raise NotImplementedError("rendering is out of scope")

    def render(self, mode="human"):
        raise NotImplementedError("rendering is out of scope")

    def _indices(self, indices):
        if indices is None:
            return list(range(self.num_envs))
        if isinstance(indices, int):
            return [indices]
        return list(indices)


class HipGymEnv:
    """Single ReachHuman env with the gym-0.21 API: `reset() -> obs`, `step(a) -> (obs, reward, done, info)`.

    Stepping a finished episode raises ValueError like HumanEnv.step (human_env.py:487-488)."""

    def __init__(self, env_kwargs=None, seed=None, clips=None, device=0, backend=None, obs_keys=None, collision_prevention=None,
                 env_id="ReachHuman"):
        self._vec = HipVecEnv(1, env_id=env_id, env_kwargs=env_kwargs, seed=seed, clips=clips, device=device, backend=backend, obs_keys=obs_keys,
                              collision_prevention=collision_prevention)
        self.observation_space = self._vec.observation_space
        self.action_space = self._vec.action_space
        self._done = True
        self._next_obs = None

    def reset(self):
        if self._next_obs is not None:  # the kernel already reset the env when the episode ended
            obs, self._next_obs = self._next_obs, None
        else:
            obs = self._vec.reset()[0]
        self._done = False
        return obs

    def step(self, action):
        if self._done:
            raise ValueError("executing action in terminated episode")
        obs, rew, done, infos = self._vec.step(np.asarray(action, np.float64)[None])
        info = infos[0]
        if done[0]:
            self._done = True
            self._next_obs = obs[0]
            return info["terminal_observation"], float(rew[0]), True, info
        return obs[0], float(rew[0]), False, info

    def observation_dict(self, obs):
        """Split a flat observation back into the reference's observable / modality keys."""
        out, k0 = OrderedDict(), 0
        cols_of = task_columns(self._vec.env_id)   # (as HipVecEnv put the row together: a task's keys can be narrower than the superset's)
        for key in self._vec.obs_keys:
            n = len(cols_of[key])
            out[key] = obs[k0:k0 + n]
            k0 += n
        return out

    def close(self):
        self._vec.close()
