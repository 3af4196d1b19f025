"""Mixed-task batches: several tasks of the reference's experiment suite stepped side by side on one GPU.

The reference runs its ICRA-2024 task suite as separate trainings, one SubprocVecEnv per task
(`training/icra_2024_run_experiments.sh:4-9`); BASELINE.json's last configuration batches the tasks together.  A task is a
compile-time kernel variant here (hrg_step_kernel / _box / _ho), so a mixed batch is one `HipBatch` per task writing row slices of
ONE packed output block (one all-gather for N > 1 GPUs, one D2H copy for the VecEnv), each launched on its own HIP stream so that
the variants fill the chip together instead of one after the other."""
import numpy as np

from ._cstruct import CONST
from ._lib import HipBatch, as_actions
from .animation import synthetic_clips
from .model import build_model_desc
from .tasks import TASKS, value

# training/icra_2024_run_experiments.sh:4-9 (horizons as there) with the environment blocks of training/config_icra_2024/environment_evaluation/training/<task>-SAC.yaml: where
# those differ from the task's general training config (ENV_DEFAULTS) the experiment's value is listed here (tests/test_assets.py compares every common keyword)
ICRA_TASKS = (
    ("ReachHuman", dict(horizon=100, shield_type="SSM", reward_shaping=True)),
    ("PickPlaceHumanCart", dict(horizon=1000, shield_type="SSM", done_at_success=True)),
    ("CollaborativeLiftingCart", dict(horizon=5000, shield_type="SSM")),
    ("RobotHumanHandoverCart", dict(horizon=1000, shield_type="PFL", collision_reward=0)),
    ("HumanRobotHandoverCart", dict(horizon=1000, shield_type="PFL", collision_reward=0)),
    ("CollaborativeStackingCart", dict(horizon=3000, shield_type="SSM")),
)


# ... and with the one task of the reference that is not part of that suite (CollaborativeHammeringCart has no experiment config): every task the stepper covers
ALL_TASKS = ICRA_TASKS + (("CollaborativeHammeringCart", dict(horizon=1000, shield_type="SSM")),)
# ms per 4096-env step of each task's kernel alone (profiles/r03t_tasks_summary.md): the mixed batch launches its kernels longest first.  The batch is bound by LDS residency
# (the tasks' LDS images exceed the chip's 41 MB), so the order matters by 5 - 10 %, but which order wins did not reproduce from one GPU box to the next (round 2: a search over
# all 720 orders and an A/B/A/B run, "short kernels first" 5.33 vs 5.60 ms on one box and 5.95 vs 5.71 ms on another).  Longest first is the order that was never the worst.
_STEP_MS = {"CollaborativeHammeringCart": 11.5, "CollaborativeStackingCart": 6.27, "RobotHumanHandoverCart": 4.28, "HumanRobotHandoverCart": 3.93, "CollaborativeLiftingCart": 2.66,
            "HumanObjectInspectionCart": 2.43, "PickPlaceHumanCart": 1.67, "ReachHuman": 1.00}


def task_clips(env_id, n_clips=13, seed=0, **kw):
    """Synthetic clip set carrying the animation info `env_id` reads."""
    return synthetic_clips(n_clips, seed=seed, **value(TASKS[env_id].clip_extra), **kw)


def task_env_kwargs(env_id):
    """Environment keyword arguments that go with the synthetic clips of `task_clips` (the reference's defaults belong to its recorded clips)."""
    return value(TASKS[env_id].clip_env_kwargs)


def split_evenly(n_envs, n_tasks):
    """Env counts per task: as even as possible, the remainder to the first tasks."""
    q, r = divmod(int(n_envs), int(n_tasks))
    return [q + (1 if i < r else 0) for i in range(n_tasks)]


class MixedBatch:
    """`parts`: list of (env_id, desc, clips, n_envs).  Rows of every output are ordered part by part; `slices[i]` is part i's row range."""

    def __init__(self, parts, env_id0=0, device=0, concurrent=True):
        import torch
        from .dist import packed_layout, packed_views
        if not torch.cuda.is_available():
            raise RuntimeError("MixedBatch needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.n = sum(int(p[3]) for p in parts)
        lay = packed_layout(self.n)
        self.packed = torch.zeros(lay["total"], dtype=torch.uint8, device=self.device)
        self.packed_head = self.packed[:lay["head"]]
        v = packed_views(self.packed, self.n)
        self.obs, self.term_obs, self.reward, self.info, self.done = v["obs"], v["term_obs"], v["reward"], v["info"], v["done"]
        self.env_ids, self.slices, self.batches = [], [], []
        r0 = 0
        for env_id, desc, clips, k in parts:
            sl = slice(r0, r0 + int(k))
            out = (self.obs[sl], self.term_obs[sl], self.reward[sl], self.info[sl], self.done[sl])
            self.batches.append(HipBatch(desc, clips, int(k), env_id0=env_id0 + r0, device=device, out=out))
            self.env_ids.append(env_id)
            self.slices.append(sl)
            r0 += int(k)
        self.concurrent = bool(concurrent) and len(parts) > 1
        # launch the long kernels first: the step ends with the last kernel to finish, and a kernel launched late queues behind the others for wave slots and LDS (see _STEP_MS)
        self._launch_order = sorted(range(len(parts)), key=lambda i: -_STEP_MS.get(parts[i][0], 2.1) * int(parts[i][3]))
        with torch.cuda.device(self.device):
            self.streams = [torch.cuda.Stream() for _ in parts] if self.concurrent else None   # (high-priority streams for the long kernels: no effect, 8.46 vs 8.47 ms)

    def _each(self, fn):
        t = self.torch
        if not self.concurrent:
            for i, b in enumerate(self.batches):
                fn(i, b)
            return
        cur = t.cuda.current_stream(self.device)
        for i in self._launch_order:
            b, s = self.batches[i], self.streams[i]
            s.wait_stream(cur)          # inputs written on the caller's stream
            with t.cuda.stream(s):
                fn(i, b)
        for s in self.streams:
            cur.wait_stream(s)          # outputs are consumed on the caller's stream

    def reset(self, mask=None):
        self._each(lambda i, b: b.reset(None if mask is None else mask[self.slices[i]]))
        return self.obs

    def step(self, actions):
        """actions: float64 [n, 7] on the device (rows in part order).  Returns (obs, reward, done, info) views of the shared block."""
        actions = as_actions(actions, self.n, self.device)
        self._each(lambda i, b: b.step(actions[self.slices[i]]))
        self._keep = actions
        return self.obs, self.reward, self.done, self.info

    def kernel_time(self):
        """(sum over the parts of their average step-kernel ms, launches per part) since the previous call; the first call arms the timers.
        With `concurrent` the kernels overlap, so the sum exceeds the step's wall time."""
        per = [b.kernel_time() for b in self.batches]
        return sum(ms for ms, _ in per), (per[0][1] if per else 0)

    def part_of(self, env):
        """(part index, row within the part) of global row `env`."""
        for i, sl in enumerate(self.slices):
            if sl.start <= env < sl.stop:
                return i, env - sl.start
        raise IndexError(env)

    def get_state(self, e):
        i, r = self.part_of(e)
        return self.batches[i].get_state(r)

    def close(self):
        for b in self.batches:
            b.close()
        self.batches = []


def make_mixed_batch(n_envs, tasks=ICRA_TASKS, env_kwargs=None, clips=None, n_clips=13, seed=None, env_id0=0, device=0, concurrent=True, robot_geometry="capsule"):
    """`n_envs` environments split evenly over `tasks` = [(env_id, kwargs), ...]; `env_kwargs` are applied to every task first.
    `robot_geometry` ("capsule" | "hull", see `build_model_desc`) goes to every part."""
    counts = split_evenly(n_envs, len(tasks))
    parts = []
    for (env_id, kw), k in zip(tasks, counts):
        if k == 0:
            continue
        kw = dict(task_env_kwargs(env_id), **dict(env_kwargs or {}, **kw))
        if seed is not None:
            kw["seed"] = int(seed)
        c = (clips or {}).get(env_id) if isinstance(clips, dict) else None
        c = c if c is not None else task_clips(env_id, n_clips)
        parts.append((env_id, build_model_desc(kw, n_clips=c.n_clips, env_id=env_id, robot_geometry=robot_geometry), c, k))
    return MixedBatch(parts, env_id0=env_id0, device=device, concurrent=concurrent)


def make_mixed_vec_env(n_envs, tasks=ICRA_TASKS, obs_keys=None, env_kwargs=None, seed=None, start_index=0, clips=None, n_clips=13,
                       device=0, info_dicts=True, concurrent=True, robot_geometry="capsule", expert=None, imitation_reward=None, dataset=None, rsi_prob=None,
                       state_imitation_reward=None):
    """A `HipVecEnv`-shaped VecEnv over a mixed batch.  One policy sees every task, so the observation is the same columns for all
    of them: `obs_keys` (names valid for every task) or, by default, the whole 64-column observation superset (columns a task does
    not fill are zero).  `infos[i]["task"]` names the task of row i; `env.task_slices` maps env ids to row ranges.
    `robot_geometry` as in `make_mixed_batch`."""
    if expert is not None or imitation_reward is not None:
        raise NotImplementedError("expert / imitation_reward: scripted experts are per task and action form; use one HipVecEnv(expert=...) per task")
    if dataset is not None or rsi_prob is not None or state_imitation_reward is not None:
        raise NotImplementedError("dataset / rsi_prob / state_imitation_reward: a demonstration dataset is per task; use one HipVecEnv(dataset=...) per task")
    batch = make_mixed_batch(n_envs, tasks, env_kwargs=env_kwargs, clips=clips, n_clips=n_clips, seed=seed, env_id0=start_index,
                             device=device, concurrent=concurrent, robot_geometry=robot_geometry)
    return __getattr__("MixedHipVecEnv")(batch, obs_keys=obs_keys, info_dicts=info_dicts)


def _mixed_cls():
    from .vec_env import OBS_COLUMNS, HipVecEnv, _TorchBackend

    class MixedHipVecEnv(HipVecEnv):
        """VecEnv over a `MixedBatch` (see `make_mixed_vec_env`).  Joint-space actions [n, 7] for every task.  `batch`: the MixedBatch, or any backend
        (protocol: vec_env._TorchBackend) that carries its parts' `env_ids` and row `slices`."""

        def __init__(self, batch, obs_keys=None, info_dicts=True):
            n = sum(sl.stop - sl.start for sl in batch.slices)
            self.env_id = "mixed(" + ",".join(batch.env_ids) + ")"
            self.task_slices = dict(zip(batch.env_ids, batch.slices))
            self._task_of_row = [eid for eid, sl in zip(batch.env_ids, batch.slices) for _ in range(sl.stop - sl.start)]
            self._init_dataset()    # the steps of HipVecEnv.__init__, without the per-task wrappers: no dataset, no expert, no action front-end
            self._init_expert()
            self._init_columns(obs_keys, OBS_COLUMNS)
            self._backend = batch if hasattr(batch, "step_async") else _TorchBackend(batch=batch)
            self._init_spaces(n)
            self._init_accounting(n, info_dicts)
            self._init_obs_norm()
            self._init_monitor()

        def _make_infos(self, info, dones, term_obs, sir=None):
            infos = super()._make_infos(info, dones, term_obs, sir)
            for d, task in zip(infos, self._task_of_row):
                dict.__setitem__(d, "task", task)   # (not d[...] = ...: that would fill the lazy rows)
            return infos

        def seed(self, seed=None):
            raise NotImplementedError("re-seeding a mixed batch: build a new one with make_mixed_vec_env(seed=...)")

        def get_attr(self, attr_name, indices=None):
            if attr_name == "task":
                return [self._task_of_row[i] for i in self._indices(indices)]
            if attr_name == "joint_pos":
                return HipVecEnv.get_attr(self, attr_name, indices)
            raise AttributeError(f"MixedHipVecEnv has no per-env attribute {attr_name!r}")

        def compute_reward(self, *a, **k):
            raise NotImplementedError("goal-env relabelling is per task; use one HipVecEnv(goal_env=True) per task")

        def compute_done(self, *a, **k):
            raise NotImplementedError("goal-env relabelling is per task; use one HipVecEnv(goal_env=True) per task")

        def attach_her(self, *a, **k):
            raise NotImplementedError("goal-env relabelling is per task; use one HipVecEnv(goal_env=True) per task")

        def device_refusal(self, kind):
            return {"rollout": "the mixed batch steps one HipBatch per task", "replay": "the mixed batch has its observation columns per task",
                    "demonstrations": "a demonstration dataset is per task", "dagger": "scripted experts are per task and action form",
                    "discriminator": "a demonstration dataset is per task"}.get(kind, "goal-env relabelling is per task") + "; use one HipVecEnv per task"

        def expert_actions(self):
            raise NotImplementedError("scripted experts are per task and action form; use one HipVecEnv(expert=...) per task")

    return MixedHipVecEnv


def __getattr__(name):
    if name == "MixedHipVecEnv":
        cls = _mixed_cls()
        globals()["MixedHipVecEnv"] = cls
        return cls
    raise AttributeError(name)
