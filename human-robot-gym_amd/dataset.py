"""Demonstration datasets for the batched stepper: file format, collector, and the keyword dicts -> `hrg_dataset_desc` (include/hrgym.h).

The reference records one folder per episode (`ep_XXXX/state.npz` + `model.xml`, training/create_expert_dataset.py with DatasetCollectionWrapper) and
loads them all in DatasetWrapper.load_dataset (wrappers/dataset_wrapper.py:43-85).  Here a dataset is ONE file, `datasets/<dataset_name>/hrg_dataset.npz`,
with the episodes concatenated:

  ep_offset[n_ep + 1] int64     episode k has T_k = ep_offset[k + 1] - ep_offset[k] transitions
  states[total_T, hrg_state_bytes()] uint8   raw bytes of hrg_env_state BEFORE transition t
  boxes[total_T, hrg_box_bytes()] uint8      raw bytes of hrg_box_state; present exactly when the task has a box block
  obs[total_T + n_ep, 64] float32            per episode rows 0 .. T_k of the observation superset; row T_k is the terminal observation
  actions[total_T, HRG_ACT_DIM] float64      the expert's action rows as commanded (before the IK front-end / collision prevention rewrite them)
  ep_return[n_ep], ep_success[n_ep]          statistics only
  header: env_id, state_bytes, box_bytes, version, robot_geometry, cartesian, obs_keys

The state AFTER the last transition is not stored: the step kernel has auto-reset the block by then, and nothing reads it (the reference draws its start
step with np.random.randint(T) < T, dataset_wrapper.py:155).  The kernels that consume a dataset are in csrc/hrgym_dataset.h.
"""
import ctypes
import os

import numpy as np

from ._cstruct import CONST, BoxState, DatasetDesc, EnvState
from .tasks import TASKS, task_row

FILE_NAME = "hrg_dataset.npz"
STATE_BYTES, BOX_BYTES = ctypes.sizeof(EnvState), ctypes.sizeof(BoxState)
SIR_KINDS = {env_id: t.sir for env_id, t in TASKS.items() if t.sir is not None}   # StateBasedExpertImitationRewardWrapper subclass per task
SIR_COLUMNS = ("r_im", "r_env", "r_motion", "r_gripper", "r_full", "ep_im", "ep_env", "ep_motion", "ep_gripper", "ep_len", "ep_len_mg", "early", "time",
               "time_obs")   # HRG_SIR_*
_SIM_FNS = {"gaussian": CONST["HRG_SIM_GAUSSIAN"], "tanh": CONST["HRG_SIM_TANH"]}
# constructor arguments of the wrappers (334-346, 486-501, 672-684) without env, dataset_name, rsi_prob, verbose
_SIR_COMMON = dict(alpha=0.0, observe_time=True, use_et=False, et_dist=2.0)
_SIR_SINGLE = dict(_SIR_COMMON, iota=0.1, sim_fn="gaussian")
_SIR_PICK_PLACE = dict(_SIR_COMMON, beta=0.0, iota_m=0.1, iota_g=0.05, m_sim_fn="gaussian", g_sim_fn="gaussian")
DEFAULT_CAPACITY_BYTES = 2 << 30


def library_version():
    from ._lib import load_library
    return load_library().hrg_version().decode()


def check_holds_state(env_id):
    """A dataset holds (hrg_env_state, hrg_box_state) per transition: refuse a task whose state lives in a further array (hrg_stack_state, hrg_hammer_state)."""
    if TASKS[env_id].block in ("stack", "hammer"):
        raise NotImplementedError(f"dataset: {env_id} keeps its state in further arrays (hrg_stack_state / hrg_hammer_state), which a dataset does not hold")


def dataset_path(name_or_path):
    """`datasets/<dataset_name>/hrg_dataset.npz` (relative to the working directory, like the existing datasets/<name>/observations.csv), or the path itself."""
    p = str(name_or_path)
    if p.endswith(".npz"):
        return p
    return os.path.join("datasets", p, FILE_NAME)


def sir_kwargs(env_id, state_imitation_reward):
    """`state_imitation_reward` dict -> the wrapper's arguments in the two-term form (alpha, beta, iota_m, iota_g, m_sim_fn, g_sim_fn, observe_time,
    use_et, et_dist).  The Reach / Lifting wrappers take `iota` / `sim_fn` (their one term is the motion term); unknown arguments raise."""
    if env_id not in SIR_KINDS:
        raise NotImplementedError(f"state_imitation_reward: the reference has no state-based imitation reward wrapper for {env_id} (available {sorted(SIR_KINDS)})")
    kw = dict(state_imitation_reward)
    for k in ("rsi_prob", "dataset_name", "verbose"):
        kw.pop(k, None)
    single = SIR_KINDS[env_id] != CONST["HRG_SIR_PICK_PLACE"]
    known = _SIR_SINGLE if single else _SIR_PICK_PLACE
    unknown = sorted(set(kw) - set(known))
    if unknown:
        raise TypeError(f"state_imitation_reward ({env_id}): unexpected arguments {unknown} (the wrapper takes {sorted(known)})")
    v = {k: kw.get(k, d) for k, d in known.items()}
    out = dict(alpha=float(v["alpha"]), observe_time=bool(v["observe_time"]), use_et=bool(v["use_et"]), et_dist=float(v["et_dist"]))
    if single:
        out.update(beta=1.0, iota_m=float(v["iota"]), iota_g=1.0, m_sim_fn=v["sim_fn"], g_sim_fn="gaussian")
    else:
        out.update(beta=float(v["beta"]), iota_m=float(v["iota_m"]), iota_g=float(v["iota_g"]), m_sim_fn=v["m_sim_fn"], g_sim_fn=v["g_sim_fn"])
    for k in ("m_sim_fn", "g_sim_fn"):
        if out[k] not in _SIM_FNS:
            raise ValueError(f"Unknown similarity function: {out[k]}")
    return out


class ExpertDataset:
    """A loaded demonstration dataset (see the module docstring for the fields)."""

    def __init__(self, env_id, ep_offset, states, obs, actions, boxes=None, robot_geometry="capsule", cartesian=False, obs_keys=(), ep_return=None, ep_success=None,
                 version=None):
        self.env_id = str(env_id)
        self.ep_offset = np.ascontiguousarray(ep_offset, np.int64)
        self.states = np.ascontiguousarray(states, np.uint8)
        self.boxes = None if boxes is None else np.ascontiguousarray(boxes, np.uint8)
        self.obs = np.ascontiguousarray(obs, np.float32)
        self.actions = np.ascontiguousarray(actions, np.float64)
        self.robot_geometry, self.cartesian, self.obs_keys = str(robot_geometry), bool(cartesian), [str(k) for k in obs_keys]
        n = self.n_episodes
        self.ep_return = np.zeros(n) if ep_return is None else np.asarray(ep_return, np.float64)
        self.ep_success = np.zeros(n, bool) if ep_success is None else np.asarray(ep_success, bool)
        self.version = library_version() if version is None else str(version)
        self.validate()

    n_episodes = property(lambda self: len(self.ep_offset) - 1)
    total_T = property(lambda self: int(self.ep_offset[-1]))

    def T(self, k):
        return int(self.ep_offset[k + 1] - self.ep_offset[k])

    def obs_row0(self, k):
        """Index of episode k's first observation row (every episode carries one row more than it has transitions)."""
        return int(self.ep_offset[k]) + k

    def episode(self, k):
        a, b, r = int(self.ep_offset[k]), int(self.ep_offset[k + 1]), self.obs_row0(k)
        return dict(states=self.states[a:b], boxes=None if self.boxes is None else self.boxes[a:b], obs=self.obs[r:r + (b - a) + 1], actions=self.actions[a:b])

    def select(self, episodes, lengths=None):
        """A dataset of the listed episodes, each cut to its first lengths[i] transitions (default: whole).  A shortened episode's last observation row is
        the one its next transition started from."""
        lengths = [self.T(k) for k in episodes] if lengths is None else [int(x) for x in lengths]
        if any(not 1 <= n <= self.T(k) for k, n in zip(episodes, lengths)):
            raise ValueError("select: every length must lie in [1, T of its episode]")
        parts = [dict((key, None if v is None else v[:n + (key == "obs")]) for key, v in self.episode(k).items()) for k, n in zip(episodes, lengths)]
        cat = lambda key: np.concatenate([p[key] for p in parts])   # noqa: E731
        return ExpertDataset(self.env_id, np.concatenate([[0], np.cumsum(lengths)]), cat("states"), cat("obs"), cat("actions"),
                             boxes=None if self.boxes is None else cat("boxes"), robot_geometry=self.robot_geometry, cartesian=self.cartesian, obs_keys=self.obs_keys,
                             ep_return=self.ep_return[list(episodes)], ep_success=self.ep_success[list(episodes)], version=self.version)

    def validate(self):
        eo = self.ep_offset
        if eo.ndim != 1 or len(eo) < 2 or eo[0] != 0 or np.any(np.diff(eo) <= 0):
            raise ValueError("dataset: ep_offset must start at 0 and every episode needs at least one transition")
        tt, n = self.total_T, self.n_episodes
        if self.states.shape != (tt, STATE_BYTES):
            raise ValueError(f"dataset: states of shape {self.states.shape}, expected {(tt, STATE_BYTES)} (hrg_state_bytes)")
        if self.boxes is not None and self.boxes.shape != (tt, BOX_BYTES):
            raise ValueError(f"dataset: boxes of shape {self.boxes.shape}, expected {(tt, BOX_BYTES)} (hrg_box_bytes)")
        if self.obs.shape != (tt + n, CONST["HRG_OBS_DIM"]) or self.actions.shape != (tt, CONST["HRG_ACT_DIM"]):
            raise ValueError(f"dataset: obs {self.obs.shape} / actions {self.actions.shape} do not fit {tt} transitions in {n} episodes")

    def restore_states(self):
        """The state blocks as they are uploaded for reference state initialisation: the recorded bytes with `timestep` (policy steps of the episode, what the
        time limit counts) set to zero.  In the reference TimeLimit.reset() zeroes its counter before DatasetRSIWrapper restores the state and
        set_environment_state does not touch it or env.timestep (time_limit.py:46-49, human_env.py:1862-1900): a restored episode gets the whole horizon."""
        s = self.states.copy()
        off = EnvState.timestep.offset
        s[:, off:off + 4] = 0
        return s

    def save(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        data = dict(ep_offset=self.ep_offset, states=self.states, obs=self.obs, actions=self.actions, ep_return=self.ep_return, ep_success=self.ep_success,
                    env_id=np.array(self.env_id), state_bytes=np.int64(STATE_BYTES), box_bytes=np.int64(BOX_BYTES), version=np.array(self.version),
                    robot_geometry=np.array(self.robot_geometry), cartesian=np.bool_(self.cartesian), obs_keys=np.array(self.obs_keys, dtype=str))
        if self.boxes is not None:
            data["boxes"] = self.boxes
        np.savez_compressed(path, **data)
        return path

    @classmethod
    def load(cls, name_or_path, env_id=None, has_box=None, version=None):
        """Load `datasets/<name>/hrg_dataset.npz` (or a path).  A header that does not fit is refused: another state or box size, another library version
        (`version`: default the loaded library's), another task than `env_id`, a box array that is there / missing against `has_box`."""
        path = dataset_path(name_or_path)
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
        if int(d["state_bytes"]) != STATE_BYTES or int(d["box_bytes"]) != BOX_BYTES:
            raise ValueError(f"{path}: recorded with hrg_state_bytes = {int(d['state_bytes'])}, hrg_box_bytes = {int(d['box_bytes'])}; this build has {STATE_BYTES}, {BOX_BYTES}")
        want = library_version() if version is None else version
        if str(d["version"]) != want:
            raise ValueError(f"{path}: recorded by {str(d['version'])!r}; this library is {want!r}")
        if env_id is not None and str(d["env_id"]) != env_id:
            raise ValueError(f"{path}: a dataset of {str(d['env_id'])}, not of {env_id}")
        if has_box is not None and ("boxes" in d) != bool(has_box):
            raise ValueError(f"{path}: the dataset {'has' if 'boxes' in d else 'has no'} box array; the task {'has' if has_box else 'has no'} box block")
        return cls(str(d["env_id"]), d["ep_offset"], d["states"], d["obs"], d["actions"], boxes=d.get("boxes"), robot_geometry=str(d["robot_geometry"]),
                   cartesian=bool(d["cartesian"]), obs_keys=[str(k) for k in d["obs_keys"]], ep_return=d["ep_return"], ep_success=d["ep_success"], version=str(d["version"]))


def build_dataset_desc(dataset, rsi_prob=0.0, state_imitation_reward=None, seed=0):
    """hrg_dataset_desc of `dataset` (+ the arguments of sir_kwargs): returns (desc, keepalive) -- the descriptor points into the host arrays of `keepalive`."""
    d = DatasetDesc()
    keep = [np.ascontiguousarray(dataset.ep_offset, np.int64), dataset.restore_states(), None if dataset.boxes is None else np.ascontiguousarray(dataset.boxes),
            np.ascontiguousarray(dataset.obs, np.float32)]
    d.n_episodes, d.total_T = dataset.n_episodes, dataset.total_T
    d.ep_offset, d.states, d.obs = keep[0].ctypes.data, keep[1].ctypes.data, keep[3].ctypes.data
    d.boxes = keep[2].ctypes.data if keep[2] is not None else None
    d.rsi_prob = float(rsi_prob or 0.0)
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d.sir_kind = CONST["HRG_SIR_NONE"]
    d.iota_m = d.iota_g = 1.0
    if state_imitation_reward is not None:
        r = sir_kwargs(dataset.env_id, state_imitation_reward)
        d.sir_kind = SIR_KINDS[dataset.env_id]
        d.use_et = int(r["use_et"])
        d.alpha, d.beta, d.iota_m, d.iota_g, d.et_dist = r["alpha"], r["beta"], r["iota_m"], r["iota_g"], r["et_dist"]
        d.m_sim_fn, d.g_sim_fn = _SIM_FNS[r["m_sim_fn"]], _SIM_FNS[r["g_sim_fn"]]
    return d, keep


def cut_episodes(done, n_episodes=None):
    """Cut every env's tape at its done flags: `done` bool [steps, n_envs] -> list of (env, first step, last step) of the finished episodes in (env, episode)
    order, the first `n_episodes` of them.  What an env recorded after its last done flag (an episode it never finished) is dropped."""
    done = np.asarray(done, bool)
    out = []
    for e in range(done.shape[1]):
        t0 = 0
        for t in np.nonzero(done[:, e])[0].tolist():
            out.append((e, t0, t))
            t0 = t + 1
    return out if n_episodes is None else out[:int(n_episodes)]


def tape_bytes(n_steps, n_envs, has_box):
    """Device memory of a collector tape: per env and step the state block, the box block, two observation rows, the action row, reward, done, successes."""
    row = STATE_BYTES + (BOX_BYTES if has_box else 0) + 2 * 4 * CONST["HRG_OBS_DIM"] + 8 * CONST["HRG_ACT_DIM"] + 4 + 1 + 4
    return int(n_steps) * int(n_envs) * row


def assemble(env_id, episodes, states, boxes, obs, term_obs, actions, reward, success, **header):
    """Host arrays of a tape ([steps, n_envs, ...]) + the cut list -> ExpertDataset."""
    ep_offset = np.zeros(len(episodes) + 1, np.int64)
    S, B, O, A, ret, suc = [], [], [], [], [], []
    for k, (e, t0, t1) in enumerate(episodes):
        ep_offset[k + 1] = ep_offset[k] + (t1 - t0 + 1)
        S.append(states[t0:t1 + 1, e])
        if boxes is not None:
            B.append(boxes[t0:t1 + 1, e])
        O.append(obs[t0:t1 + 1, e])
        O.append(term_obs[t1:t1 + 1, e])
        A.append(actions[t0:t1 + 1, e])
        ret.append(float(np.sum(reward[t0:t1 + 1, e], dtype=np.float64)))
        suc.append(bool(success[t1, e]))
    return ExpertDataset(env_id, ep_offset, np.concatenate(S), np.concatenate(O), np.concatenate(A), boxes=np.concatenate(B) if boxes is not None else None,
                         ep_return=ret, ep_success=suc, **header)


def write_stats(dataset, folder, cols):
    """observations.csv: mean / std per policy-visible observation value over every recorded observation (create_expert_dataset.py:147-161; read back by
    wrappers.dataset_obs_norm); stats.csv: the columns of compute_stats (86-106) that need no bootstrap."""
    os.makedirs(folder, exist_ok=True)
    v = dataset.obs[:, list(cols)].astype(np.float64)
    with open(os.path.join(folder, "observations.csv"), "w") as f:
        f.write("mean,std\n")
        for m, s in zip(v.mean(axis=0), v.std(axis=0)):
            f.write(f"{float(m)!r},{float(s)!r}\n")
    lens = np.diff(dataset.ep_offset).astype(np.float64)
    with open(os.path.join(folder, "stats.csv"), "w") as f:
        f.write("success_mean,ep_len_mean,ep_len_std,ep_rew_mean,ep_rew_std\n")
        f.write(",".join(repr(float(x)) for x in (dataset.ep_success.mean(), lens.mean(), lens.std(), dataset.ep_return.mean(), dataset.ep_return.std())) + "\n")


def collect_expert_dataset(env_id, n_episodes, n_envs, expert, dataset_name=None, max_steps=None, capacity_bytes=DEFAULT_CAPACITY_BYTES, **env_kwargs):
    """Record `n_episodes` demonstration episodes of the scripted `expert` (dict(id=..., ...)) on `n_envs` batched envs (training/create_expert_dataset.py).

    `env_kwargs` are HipVecEnv's keyword arguments (env_kwargs=, seed=, ik_position_delta=, robot_geometry=, obs_keys=, ...).  Every step the whole state
    array is snapshotted on the device before it is stepped with the expert's actions; the tape stays on the device until the run ends.  Then each env's
    tape is cut at its done flags and the first `n_episodes` finished episodes in (global env id, episode) order are kept -- all of them, like the
    reference: success is a statistic, not a filter.  `max_steps` defaults to ceil(n_episodes / n_envs) x horizon, by which every env has finished that
    many episodes.  Raises before allocating when the tape exceeds `capacity_bytes`.  With `dataset_name` the dataset and its statistics files are
    written to datasets/<dataset_name>/.  Returns the ExpertDataset."""
    import torch
    from .vec_env import HipVecEnv
    check_holds_state(env_id)
    has_box = task_row(env_id, bool(env_kwargs.get("reach_box"))).block == "box"
    horizon = int((env_kwargs.get("env_kwargs") or {}).get("horizon", TASKS[env_id].env_kwargs["horizon"]))
    steps = int(max_steps) if max_steps is not None else -(-int(n_episodes) // int(n_envs)) * horizon
    need = tape_bytes(steps, n_envs, has_box)
    if need > capacity_bytes:   # before anything is allocated, the batch included
        raise MemoryError(f"collect_expert_dataset: a tape of {steps} steps x {n_envs} envs takes {need} bytes, more than capacity_bytes = {capacity_bytes}; "
                          "use fewer envs or steps, or collect in several runs")
    env = HipVecEnv(n_envs, env_id=env_id, expert=expert, info_dicts=False, **env_kwargs)
    try:
        batch = env._backend.batch
        dev, od, ad = batch.device, CONST["HRG_OBS_DIM"], CONST["HRG_ACT_DIM"]
        t_states = torch.empty(steps, n_envs, STATE_BYTES, dtype=torch.uint8, device=dev)
        t_boxes = torch.empty(steps, n_envs, BOX_BYTES, dtype=torch.uint8, device=dev) if has_box else None
        t_obs, t_term = torch.empty(steps, n_envs, od, dtype=torch.float32, device=dev), torch.zeros(steps, n_envs, od, dtype=torch.float32, device=dev)
        t_act = torch.empty(steps, n_envs, ad, dtype=torch.float64, device=dev)
        t_rew, t_done = torch.empty(steps, n_envs, dtype=torch.float32, device=dev), torch.empty(steps, n_envs, dtype=torch.uint8, device=dev)
        t_goal = torch.empty(steps, n_envs, dtype=torch.int32, device=dev)
        batch.reset()
        for t in range(steps):
            batch.snapshot(t_states[t], t_boxes[t] if has_box else None)
            t_obs[t].copy_(batch.obs)
            t_act[t].copy_(batch.expert_actions())
            obs, rew, done, info = batch.step(t_act[t].clone())   # the step rewrites its action rows (IK front-end, collision prevention): the tape keeps the command
            t_term[t].copy_(batch.term_obs)
            t_rew[t].copy_(rew)
            t_done[t].copy_(done)
            t_goal[t].copy_(info[:, CONST["HRG_INFO_N_GOAL_REACHED"]])
        torch.cuda.synchronize(dev)
        done = t_done.cpu().numpy() != 0
        episodes = cut_episodes(done, n_episodes)
        if len(episodes) < int(n_episodes):
            raise RuntimeError(f"collect_expert_dataset: {len(episodes)} episodes finished in {steps} steps, {n_episodes} asked for (raise max_steps)")
        ds = assemble(env_id, episodes, t_states.cpu().numpy(), t_boxes.cpu().numpy() if has_box else None, t_obs.cpu().numpy(), t_term.cpu().numpy(),
                      t_act.cpu().numpy(), t_rew.cpu().numpy(), t_goal.cpu().numpy() > 0, robot_geometry=env._robot_geometry, cartesian=env._ik is not None,
                      obs_keys=env.obs_keys)
        if dataset_name is not None:
            folder = os.path.dirname(os.path.abspath(dataset_path(dataset_name)))
            ds.save(dataset_path(dataset_name))
            write_stats(ds, folder, env._cols)
        return ds
    finally:
        env.close()
