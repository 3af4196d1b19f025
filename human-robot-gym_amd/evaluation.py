"""Evaluation of trained policies on the device: SB3 1.5.0's `evaluate_policy(model, env, n_eval_episodes, deterministic=True)` -- the other half of the
reference's `train_and_evaluate` (utils/training_utils_SB3.py:492-611, callbacks/custom_wandb_callback.py:178-271) -- as a loop of three kernel launches per
env step: the step, the episode ledger, the fused deterministic actor (csrc/hrgym_eval.h).  No torch op and no copy to the host sits between them; the host reads
one integer every `sync_every` steps to learn whether every episode is in.

    env = create_training_vec_env(config, evaluation_mode=True)
    learner = SacLearner.load(checkpoint_path(run_id, "final"), device=0)
    result = env.evaluate(learner, n_eval_episodes=20)             # EvalResult: episode_rewards, mean_reward, std_reward, infos["n_goal_reached"], ...
    mean, std = evaluate_policy(learner, env, n_eval_episodes=20)  # SB3's calling form

What the reference cannot do: all checkpoints of a run in one batch (`load_step: all`).  The batch is split into P groups of consecutive envs, group k stepped by
row k of a stacked parameter tensor:

    stacked = torch.stack([SacLearner.load(p, device=0).p.params for _, p in list_checkpoints(run_id)])
    per_checkpoint = env.evaluate(stacked, 20, learner=learner).by_policy()

What differs from SB3: within a group the episode quotas are SB3's episode_count_targets; Monitor's return is not rounded to six decimals (as the host path's
infos["episode"]["r"]); a non-deterministic evaluation, rendering, a callback and recurrent states are refused by name."""
import ctypes
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

from ._cstruct import CONST, EvalDesc
from ._device import DeviceHandle, check_columns
from ._lib import _ptr

RECORD_DIM = CONST["HRG_EVAL_RECORD_DIM"]
MAX_EPISODES_PER_ENV = CONST["HRG_EVAL_MAX_EPISODES_PER_ENV"]
REC_RETURN, REC_LENGTH, REC_STEP, REC_TRUNCATED, REC_INFO, REC_EP_IM = (CONST["HRG_EVAL_REC_" + k] for k in ("RETURN", "LENGTH", "STEP", "TRUNCATED", "INFO", "EP_IM"))
GOAL_DIMS = {"reach": (6, 6), "cube": (7, 3)}   # achieved_goal, desired_goal (csrc/hrgym_her.h)


def quotas(n_envs, n_policies, n_eval_episodes):
    """int64 [n_envs]: the episodes each env contributes -- SB3's episode_count_targets within each of the `n_policies` groups of consecutive envs."""
    m = int(n_envs) // int(n_policies)
    return (int(n_eval_episodes) + np.arange(int(n_envs)) % m) // m


def build_eval_desc(n_envs, n_policies, n_eval_episodes, obs_cols, act_low, act_high, observe_time=False, mean=None, std=None, squash_factor=None, goal_kind=None):
    """hrg_eval_desc (include/hrgym.h).  `obs_cols`, `observe_time`, `mean` / `std` / `squash_factor`: the policy's view of a row, as replay.build_replay_desc
    takes them; `goal_kind` "reach" / "cube": the view is the feature row of a goal env instead.  `act_low` / `act_high`: the action space's bounds.  What the
    kernels do not cover is refused here, before anything is allocated or launched."""
    n_envs, n_policies, n_eval_episodes = int(n_envs), int(n_policies), int(n_eval_episodes)
    if n_envs < 1 or n_policies < 1:
        raise ValueError(f"eval: n_envs = {n_envs} and n_policies = {n_policies} must be positive")
    if n_envs % n_policies:
        raise ValueError(f"eval: n_envs = {n_envs} is not divisible by n_policies = {n_policies}: every parameter set steps a group of the same size")
    if n_eval_episodes < 1:
        raise ValueError(f"eval: n_eval_episodes = {n_eval_episodes} must be positive")
    m = n_envs // n_policies
    if -(-n_eval_episodes // m) > MAX_EPISODES_PER_ENV:
        raise ValueError(f"eval: {n_eval_episodes} episodes over groups of {m} envs are {-(-n_eval_episodes // m)} per env, above HRG_EVAL_MAX_EPISODES_PER_ENV = "
                         f"{MAX_EPISODES_PER_ENV}: use more envs")
    low, high = np.asarray(act_low, np.float64).reshape(-1), np.asarray(act_high, np.float64).reshape(-1)
    if low.shape != high.shape or not (np.isfinite(low).all() and np.isfinite(high).all() and (low <= high).all()):
        raise ValueError("eval: act_low and act_high must be finite, ordered and of one length")
    cols = check_columns("eval", obs_cols, len(low), observe_time)
    if (mean is None) != (std is None):
        raise ValueError("eval: mean and std come together")
    if squash_factor is not None and mean is None:
        raise ValueError("eval: squash_factor needs mean and std (the wrapper squashes the normalised observation)")
    d = EvalDesc()
    d.n_envs, d.n_policies, d.n_eval_episodes, d.act_dim, d.n_obs_cols, d.observe_time = n_envs, n_policies, n_eval_episodes, len(low), len(cols), int(bool(observe_time))
    for k, c in enumerate(cols):
        d.obs_cols[k] = c
    for j in range(len(low)):
        d.act_low[j], d.act_high[j] = low[j], high[j]
    if goal_kind is not None:
        if goal_kind not in GOAL_DIMS:
            raise NotImplementedError(f"eval: goal_kind = {goal_kind!r}: {sorted(GOAL_DIMS)}")
        if observe_time or mean is not None:
            raise NotImplementedError("eval: a goal env's feature row is a plain selection (no time column, no normalisation)")
        width = sum(GOAL_DIMS[goal_kind]) + len(cols)
        if width > CONST["HRG_OBS_DIM"]:
            raise NotImplementedError(f"eval: a feature row of {width} values; the kernels cover {CONST['HRG_OBS_DIM']}: construct the env with obs_keys that select fewer columns")
        d.goal_env, d.goal_kind = 1, CONST["HRG_GOAL_REACH" if goal_kind == "reach" else "HRG_GOAL_CUBE"]
    if mean is not None:
        K = len(cols) + int(bool(observe_time))
        mean, std = np.array(mean, np.float64).reshape(-1), np.array(std, np.float64).reshape(-1)
        if len(mean) != K or len(std) != K:
            raise ValueError(f"eval: statistics of length {len(mean)} / {len(std)} for an observation of length {K}")
        if not (np.isfinite(mean).all() and np.isfinite(std).all()):
            raise ValueError("eval: mean and std must be finite")
        std[std == 0] = 1   # dataset_wrapper.py:241-242
        d.normalize = 1
        for k in range(K):
            d.mean[k], d.std[k] = mean[k], std[k]
        if squash_factor is not None:
            d.squash, d.squash_factor = 1, float(squash_factor)
    return d


@dataclass
class EvalResult:
    """The episodes of an evaluation in SB3's append order -- by finishing step, then by env index: `episode_rewards` (Monitor's returns: the env's own reward) and
    `episode_lengths` as lists, `truncated` (TimeLimit.truncated at the last step), `infos` key -> float64 array over the episodes (the info columns at the
    episodes' last steps: what LoggingCallback averages under `log_info_keys`), `ep_im_rew` (the episodes' imitation reward sums), `policy` (the group of the
    env that ran the episode), `env` and `step` (the env and the finishing step since the start)."""
    episode_rewards: List[float] = field(default_factory=list)
    episode_lengths: List[int] = field(default_factory=list)
    truncated: np.ndarray = None
    infos: Dict[str, np.ndarray] = field(default_factory=dict)
    ep_im_rew: np.ndarray = None
    policy: np.ndarray = None
    env: np.ndarray = None
    step: np.ndarray = None
    n_policies: int = 1

    @property
    def mean_reward(self):
        return float(np.mean(self.episode_rewards))

    @property
    def std_reward(self):
        return float(np.std(self.episode_rewards))

    @property
    def mean_ep_length(self):
        return float(np.mean(self.episode_lengths))

    @classmethod
    def from_ledger(cls, counts, records, n_policies, info_keys):
        """The ledger of hrg_eval_export (counts int32 [n], records float64 [n, max_quota, HRG_EVAL_RECORD_DIM]) in SB3's append order."""
        counts, records = np.asarray(counts), np.asarray(records)
        n = len(counts)
        env = np.repeat(np.arange(n), counts)
        slot = np.concatenate([np.arange(c) for c in counts]) if len(env) else np.zeros(0, np.int64)   # record c of env e: its c-th finished episode
        rows = records[env, slot].reshape(-1, RECORD_DIM)
        order = np.lexsort((env, rows[:, REC_STEP]))   # the finishing step first, then the env
        rows, env = rows[order], env[order]
        return cls(episode_rewards=[float(x) for x in rows[:, REC_RETURN]], episode_lengths=[int(x) for x in rows[:, REC_LENGTH]],
                   truncated=rows[:, REC_TRUNCATED] != 0, infos={k: rows[:, REC_INFO + j].copy() for j, k in enumerate(info_keys)}, ep_im_rew=rows[:, REC_EP_IM].copy(),
                   policy=env // (n // int(n_policies)), env=env, step=rows[:, REC_STEP].astype(np.int64), n_policies=int(n_policies))

    def select(self, mask):
        """The episodes where `mask` holds, in order."""
        mask = np.asarray(mask, bool)
        return EvalResult(episode_rewards=[r for r, k in zip(self.episode_rewards, mask) if k], episode_lengths=[x for x, k in zip(self.episode_lengths, mask) if k],
                          truncated=self.truncated[mask], infos={k: v[mask] for k, v in self.infos.items()}, ep_im_rew=self.ep_im_rew[mask], policy=self.policy[mask],
                          env=self.env[mask], step=self.step[mask], n_policies=self.n_policies)

    def by_policy(self):
        """A list of EvalResult, one per parameter set, each in SB3's append order."""
        return [self.select(self.policy == k) for k in range(self.n_policies)]

    def summary(self, log_info_keys=()):
        """dict(mean_reward, std_reward, mean_ep_length, n_episodes, **means of `log_info_keys`): what the reference logs after an evaluation."""
        out = dict(mean_reward=self.mean_reward, std_reward=self.std_reward, mean_ep_length=self.mean_ep_length, n_episodes=len(self.episode_rewards))
        derived = {"ep_im_rew_mean": self.ep_im_rew, "im_rew_mean": self.ep_im_rew / np.maximum(np.asarray(self.episode_lengths, np.float64), 1.0)}
        for k in log_info_keys:
            if k not in self.infos and k not in derived:
                raise KeyError(f"log_info_keys: {k!r} is neither an info column nor an imitation reward sum ({sorted(self.infos) + sorted(derived)})")
            out[k] = float(np.mean(self.infos[k] if k in self.infos else derived[k]))
        return out


class Evaluator(DeviceHandle):
    """The episode ledger and the fused actor of one evaluation (hrg_eval_desc; `build_eval_desc`).  Owns `view` float32 [n, width], the policy's view of every
    env's current row, and `actions` float64 [n, HRG_ACT_DIM], the rows the step kernel reads.  `begin`, `step` and `policy` are asynchronous, ordered on torch's
    current stream; `remaining` and `export` synchronise."""
    _create, _destroy = "hrg_eval_create", "hrg_eval_destroy"

    def __init__(self, desc, device=0, info_keys=None):
        self._open(desc, device)
        t = self.torch
        if info_keys is None:
            from .vec_env import INFO_KEYS
            info_keys = INFO_KEYS
        self.info_keys = list(info_keys)
        self.n, self.n_policies, self.n_eval_episodes, self.act_dim = int(desc.n_envs), int(desc.n_policies), int(desc.n_eval_episodes), int(desc.act_dim)
        self.observe_time = bool(desc.observe_time)
        self.max_quota, _, self.width, _ = self._size_words()
        self.view = t.zeros(self.n, self.width, dtype=t.float32, device=self.device)
        self.actions = t.zeros(self.n, CONST["HRG_ACT_DIM"], dtype=t.float64, device=self.device)

    def _size_words(self):
        w = (ctypes.c_int64 * 4)()
        self._check(self.lib, self.lib.hrg_eval_size(self.h, w))
        return [int(x) for x in w]

    @property
    def steps(self):
        """Steps since `begin`."""
        return self._size_words()[1]

    def memory_bytes(self):
        return self._size_words()[3]

    def begin(self, obs, time=None):
        """After a reset: `obs` float32 [n, 64], `time` float32 [n] (with a time column).  Every env's count, return and length start at 0."""
        t = self.torch
        if self.observe_time and time is None:
            raise ValueError(f"begin: the observation has a time column; pass the rows' time values (float32 [{self.n}])")
        tm = self._tensor(time, t.float32, (self.n,), "time") if self.observe_time else None
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_eval_begin(self.h, self._tensor(obs, t.float32, (self.n, CONST["HRG_OBS_DIM"]), "obs"), tm, _ptr(self.view), self._stream()))

    def step(self, obs, reward, done, info, imit=None, sir=None):
        """After a step, from the tensors it wrote (`imit` / `sir`: its imitation rows, as replay.ReplayBuffer.add_step takes them): the ledger, then `view`."""
        t, C = self.torch, CONST
        args = (self._tensor(obs, t.float32, (self.n, C["HRG_OBS_DIM"]), "obs"), self._tensor(reward, t.float32, (self.n,), "reward"),
                self._tensor(done, t.uint8, (self.n,), "done"), self._tensor(info, t.int32, (self.n, C["HRG_INFO_DIM"]), "info"),
                None if imit is None else self._tensor(imit, t.float32, (self.n, C["HRG_IMIT_DIM"]), "imit"),
                None if sir is None else self._tensor(sir, t.float32, (self.n, C["HRG_SIR_DIM"]), "sir"))
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_eval_step(self.h, *args, _ptr(self.view), self._stream()))

    def policy(self, learner, params=None):
        """`actions` = the deterministic actions of `learner`'s kind (sac.SacLearner / ppo.PpoLearner) on `view`, at the env's scale: group k with row k of
        `params` float32 [n_policies, n_params] (None: the learner's own parameters, for one group).  Returns `actions`."""
        t = self.torch
        if params is None:
            params = learner.p.params.view(1, -1)
        p = self._tensor(params, t.float32, (self.n_policies, learner.p.n_params), "params")
        entry = {"hrg_sac": self.lib.hrg_eval_policy_sac, "hrg_ppo": self.lib.hrg_eval_policy_ppo}[learner._prefix]
        with t.cuda.device(self.device):
            self._check(self.lib, entry(self.h, learner.h, p, _ptr(self.view), _ptr(self.actions), self._stream()))
        self._keep = params
        return self.actions

    def remaining(self):
        """Episodes still missing, summed over the envs (synchronous: one launch, one int64 to the host)."""
        out = ctypes.c_int64(-1)
        with self.torch.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_eval_remaining(self.h, ctypes.byref(out), self._stream()))
        return int(out.value)

    def export(self):
        """(counts int32 [n], quota int32 [n], records float64 [n, max_quota, HRG_EVAL_RECORD_DIM]) on the host (synchronous)."""
        counts, quota = np.zeros(self.n, np.int32), np.zeros(self.n, np.int32)
        records = np.zeros((self.n, self.max_quota, RECORD_DIM), np.float64)
        self._check(self.lib, self.lib.hrg_eval_export(self.h, *(a.ctypes.data_as(ctypes.c_void_p) for a in (counts, quota, records))))
        return counts, quota, records

    def result(self):
        """The ledger as an EvalResult (synchronous)."""
        counts, _, records = self.export()
        return EvalResult.from_ledger(counts, records, self.n_policies, self.info_keys)


def evaluate_policy(model, env, n_eval_episodes=10, deterministic=True, render=False, callback=None, reward_threshold=None, return_episode_rewards=False, warn=True):
    """SB3's evaluate_policy for a device learner `model` on a HipVecEnv: (mean_reward, std_reward), or with `return_episode_rewards` (episode_rewards,
    episode_lengths).  `deterministic=False`, `render` and `callback` are refused: the device loop runs the deterministic actor and nothing in between."""
    if not deterministic:
        raise NotImplementedError("evaluate_policy(deterministic=False): the device loop runs the deterministic actor (the reference evaluates with deterministic=True)")
    if render:
        raise NotImplementedError("evaluate_policy(render=True): the batched envs have no renderer")
    if callback is not None:
        raise NotImplementedError("evaluate_policy(callback=...): nothing runs on the host between the steps of the device loop")
    res = env.evaluate(model, n_eval_episodes)
    if reward_threshold is not None:
        assert res.mean_reward > reward_threshold, f"Mean reward below threshold: {res.mean_reward:.2f} < {reward_threshold:.2f}"
    if return_episode_rewards:
        return res.episode_rewards, res.episode_lengths
    return res.mean_reward, res.std_reward
