"""The uniform replay buffer of SAC on flat observations on the device: SB3's `ReplayBuffer` and the bookkeeping of `OffPolicyAlgorithm._store_transition`
for a batch of envs (training/config_icra_2024/.../*-SAC.yaml: algorithm.name SAC, buffer_size, run.env_type env), plus the episode sums `Monitor` and the
imitation wrappers keep on the host.

The off-policy counterpart of `rollout.RolloutBuffer`, and `her.HerBuffer` without goals: a step's rows go into the buffer without leaving the device, as the
policy sees them -- the selected columns, the state imitation reward's time column, DatasetObsNormWrapper's normalisation (csrc/hrgym_replay.h: kernels,
layout, the draws) --, and `sample()` returns device tensors.  Storage is SB3's: time-major, slot `pos` of every env per step, the oldest slot overwritten.

    env = HipVecEnv(4096, env_id="PickPlaceHumanCart", ik_position_delta=..., collision_prevention=..., expert=..., imitation_reward=..., obs_norm=...)
    env.attach_replay(buffer_size=1_000_000)
    env.collect_steps(policy, 100)                 # train_freq steps, nothing leaves the device
    batch = env.replay.sample(256)                 # ReplayBufferSamples of device tensors
    env.replay.episode_stats()                     # dict(episodes, r, l, collision, n_goal_reached, ..., ep_im_rew): sums over the finished episodes
"""
import ctypes
from collections import namedtuple

import numpy as np

from ._cstruct import CONST, ReplayDesc
from ._device import EpisodeBuffer, check_columns
from ._lib import _ptr

# the fields SB3's SAC.train reads (stable_baselines3.common.type_aliases.ReplayBufferSamples), in its order
ReplayBufferSamples = namedtuple("ReplayBufferSamples", ["observations", "actions", "next_observations", "dones", "rewards"])

STATS_DIM = CONST["HRG_REPLAY_STATS_DIM"]   # episodes, return, length, the info columns, the imitation reward sums
INDEX_DIM = CONST["HRG_REPLAY_INDEX_DIM"]   # slot, env
# the arrays of hrg_replay_export ahead of the state word, in its order
_EXPORT_KEYS = ("observations", "next_observations", "actions", "rewards", "dones", "timeouts", "cur_obs", "cur_time", "run_return", "run_length", "stats")


def capacity_of(buffer_size, n_envs):
    """Slots of a buffer of `buffer_size` transitions over `n_envs` envs (ReplayBuffer.__init__: max(buffer_size // n_envs, 1))."""
    return max(int(buffer_size) // int(n_envs), 1)


def build_replay_desc(n_envs, buffer_size, obs_cols, act_dim=CONST["HRG_ACT_DIM"], observe_time=False, mean=None, std=None, squash_factor=None, seed=0):
    """hrg_replay_desc (include/hrgym.h).  `buffer_size`: transitions in all, as SB3 counts them.  `obs_cols`: the column of the observation superset behind
    each value of the policy's observation; `observe_time`: one more value, the time column.  `mean` / `std`: DatasetObsNormWrapper's statistics, one per value
    (time column included; std == 0 becomes 1), or both None; `squash_factor`: tanh(squash_factor * .) on top, or None."""
    n_envs, act_dim = int(n_envs), int(act_dim)
    if n_envs < 1 or int(buffer_size) < 1:
        raise ValueError(f"replay: n_envs = {n_envs} and buffer_size = {buffer_size} must be positive")
    cols = check_columns("replay", obs_cols, act_dim, observe_time)
    K = len(cols) + int(bool(observe_time))
    if (mean is None) != (std is None):
        raise ValueError("replay: mean and std come together")
    if squash_factor is not None and mean is None:
        raise ValueError("replay: squash_factor needs mean and std (the wrapper squashes the normalised observation)")
    d = ReplayDesc()
    d.n_envs, d.capacity, d.act_dim, d.n_obs_cols, d.observe_time = n_envs, capacity_of(buffer_size, n_envs), act_dim, len(cols), int(bool(observe_time))
    for k, c in enumerate(cols):
        d.obs_cols[k] = c
    if mean is not None:
        mean, std = np.array(mean, np.float64).reshape(-1), np.array(std, np.float64).reshape(-1)
        if len(mean) != K or len(std) != K:
            raise ValueError(f"replay: statistics of length {len(mean)} / {len(std)} for an observation of length {K}")
        if not (np.isfinite(mean).all() and np.isfinite(std).all()):
            raise ValueError("replay: mean and std must be finite")
        std[std == 0] = 1   # dataset_wrapper.py:241-242
        d.normalize = 1
        for k in range(K):
            d.mean[k], d.std[k] = mean[k], std[k]
        if squash_factor is not None:
            d.squash, d.squash_factor = 1, float(squash_factor)
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return d


class ReplayBuffer(EpisodeBuffer):
    """A device-resident replay buffer of `desc.capacity` slots, each one transition of every one of `desc.n_envs` envs (hrg_replay_desc;
    `build_replay_desc`).  All arguments and results are torch tensors on the buffer's device; the calls are asynchronous, ordered on torch's current
    stream (`episode_stats`, `export` and `memory_bytes` synchronise or read the handle).  `info_keys`: names of the info block's columns, for `episode_stats`."""

    _prefix, _has_time, _stats_dim = "hrg_replay", True, STATS_DIM

    def __init__(self, desc, device=0, info_keys=None):
        self._open(desc, device, info_keys)
        self.n, self.capacity, self.act_dim = int(desc.n_envs), int(desc.capacity), int(desc.act_dim)
        self.observe_time = bool(desc.observe_time)
        self.obs_dim = int(desc.n_obs_cols) + int(self.observe_time)   # K
        self.pos, self.full = 0, False   # as the handle keeps them
        self.record_index = False        # tests: keep the (slot, env) rows of the last sample() in `last_index`
        self.last_index = None

    def view(self, rows, time=None, out=None):
        """The policy's view of rows of the observation superset: float32 [m, 64] (and `time` float32 [m] when the observation has a time column) -> float32
        [m, K]: the columns, the time value, normalised and squashed as configured."""
        return self._view(rows, time, out)

    def observe(self, obs, time=None, mask=None):
        """The rows an episode starts from, after a reset: `obs` float32 [n, 64], `time` float32 [n] (with a time column); `mask` uint8 [n] (None: every
        env).  A masked env's running return and length start again."""
        self._observe(obs, time, mask)

    def add_step(self, actions, obs, term_obs, reward, done, info, imit=None, sir=None):
        """One transition per env, from the agent's actions and the tensors a step wrote: `actions` float32 [n, act_dim] at the policy's scale ([-1, 1]), `obs`
        / `term_obs` float32 [n, 64], `reward` float32 [n] (the combined reward with an imitation reward), `done` uint8 [n], `info` int32 [n, HRG_INFO_DIM];
        `imit` float32 [n, HRG_IMIT_DIM] or `sir` float32 [n, HRG_SIR_DIM]: the step's imitation rows (the env's own reward for the episode return; `sir`
        also the time columns, needed when the observation has one)."""
        t, C = self.torch, CONST
        args = (self._tensor(actions, t.float32, (self.n, self.act_dim), "actions"), self._tensor(obs, t.float32, (self.n, C["HRG_OBS_DIM"]), "obs"),
                self._tensor(term_obs, t.float32, (self.n, C["HRG_OBS_DIM"]), "term_obs"), self._tensor(reward, t.float32, (self.n,), "reward"),
                self._tensor(done, t.uint8, (self.n,), "done"), self._tensor(info, t.int32, (self.n, C["HRG_INFO_DIM"]), "info"),
                None if imit is None else self._tensor(imit, t.float32, (self.n, C["HRG_IMIT_DIM"]), "imit"),
                None if sir is None else self._tensor(sir, t.float32, (self.n, C["HRG_SIR_DIM"]), "sir"))
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_replay_add(self.h, *args, self._stream()))
        self.pos += 1
        if self.pos == self.capacity:
            self.pos, self.full = 0, True

    def add(self, *args, **kwargs):
        """Nothing: the transition went into the buffer on the device when the env stepped.  Lets the object stand where an off-policy loop expects a
        replay buffer."""

    def size(self):
        """Slots that hold a transition of every env (SB3's ReplayBuffer.size())."""
        return self.capacity if self.full else self.pos

    def sample(self, batch_size, env=None, indices=None):
        """`batch_size` transitions, slot and env drawn uniformly (SB3's sample with n_envs > 1): ReplayBufferSamples(observations [B, K], actions [B, act_dim],
        next_observations [B, K], dones [B, 1] = done * (1 - timeout), rewards [B, 1]).  `env` (SB3 passes its VecNormalize) is not used.  `indices`: int64
        [B, 2] (slot, env) pairs on the device instead of the draws (checked against the stored slots, which reads their extremes back)."""
        t = self.torch
        B = int(batch_size)
        if B < 1:
            raise ValueError("sample: batch_size must be positive")
        pi = None
        if indices is not None:
            pi = self._tensor(indices, t.int64, (B, INDEX_DIM), "indices")
            upper = self.size()
            if upper:   # (an empty buffer is the entry point's refusal)
                lo, hi = indices.min(dim=0).values.tolist(), indices.max(dim=0).values.tolist()
                if lo[0] < 0 or hi[0] >= upper or lo[1] < 0 or hi[1] >= self.n:
                    raise IndexError(f"indices: slots {lo[0]} .. {hi[0]}, envs {lo[1]} .. {hi[1]} outside the {upper} stored slots of {self.n} envs")
        new = lambda w: t.empty(B, w, dtype=t.float32, device=self.device)   # noqa: E731
        obs, act, nobs, done, rew = new(self.obs_dim), new(self.act_dim), new(self.obs_dim), new(1), new(1)
        idx = t.empty(B, INDEX_DIM, dtype=t.int64, device=self.device) if self.record_index else None
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_replay_sample(self.h, B, pi, *map(_ptr, (obs, act, nobs, done, rew, idx)), self._stream()))
        self.last_index = idx
        return ReplayBufferSamples(observations=obs, actions=act, next_observations=nobs, dones=done, rewards=rew)

    def sample_groups(self, n_groups, batch_size, seeds):
        """A population's sample: the envs are `n_groups` groups of n / n_groups consecutive envs, and group g's `batch_size` transitions come from its own
        envs under `seeds[g]` -- the draws of `sample` on a buffer of the group's envs with that seed, at the same call (a counter of this method's own).
        ReplayBufferSamples with [n_groups * batch_size, .] rows, group g's at g * batch_size.  `record_index` / `last_index` as for `sample`."""
        t = self.torch
        G, B = int(n_groups), int(batch_size)
        if G < 1 or self.n % G:
            raise ValueError(f"sample_groups: n_envs = {self.n} is not divisible by n_groups = {G}: every member samples a group of the same size")
        if B < 1:
            raise ValueError("sample_groups: batch_size must be positive")
        key = tuple(int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds)
        if len(key) != G:
            raise ValueError(f"sample_groups: {len(key)} seeds for {G} groups")
        if getattr(self, "_group_seeds", (None, None))[0] != key:   # the table the kernel reads: uploaded once per set of seeds
            self._group_seeds = (key, t.from_numpy(np.array(key, np.uint64).view(np.int64)).to(self.device))
        new = lambda w: t.empty(G * B, w, dtype=t.float32, device=self.device)   # noqa: E731
        obs, act, nobs, done, rew = new(self.obs_dim), new(self.act_dim), new(self.obs_dim), new(1), new(1)
        idx = t.empty(G * B, INDEX_DIM, dtype=t.int64, device=self.device) if self.record_index else None
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_sac_population_sample(self.h, G, B, _ptr(self._group_seeds[1]), *map(_ptr, (obs, act, nobs, done, rew, idx)), self._stream()))
        self.last_index = idx
        return ReplayBufferSamples(observations=obs, actions=act, next_observations=nobs, dones=done, rewards=rew)

    def _size_words(self):
        w = (ctypes.c_int64 * 4)()
        self._check(self.lib, self.lib.hrg_replay_size(self.h, w))
        return [int(x) for x in w]

    def memory_bytes(self):
        """Device memory the buffer holds."""
        return self._size_words()[3]

    def export(self):
        """Every array of the buffer on the host, as stored (synchronous; tests): dict of observations, next_observations [capacity, n, K], actions [capacity,
        n, act_dim], rewards, dones, timeouts [capacity, n], cur_obs [n, 64], cur_time [n], run_return, run_length [n], stats [n, HRG_REPLAY_STATS_DIM], pos,
        full, calls."""
        n, c = self.n, self.capacity
        arrays = (np.zeros((c, n, self.obs_dim), np.float32), np.zeros((c, n, self.obs_dim), np.float32), np.zeros((c, n, self.act_dim), np.float32),
                  np.zeros((c, n), np.float32), np.zeros((c, n), np.uint8), np.zeros((c, n), np.uint8), np.zeros((n, CONST["HRG_OBS_DIM"]), np.float32),
                  np.zeros(n, np.float32), np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros((n, STATS_DIM), np.float64))
        state = np.zeros(3, np.int64)
        self._check(self.lib, self.lib.hrg_replay_export(self.h, *(a.ctypes.data_as(ctypes.c_void_p) for a in arrays + (state,))))
        out = dict(zip(_EXPORT_KEYS, arrays))
        out.update(pos=int(state[0]), full=bool(state[1]), calls=int(state[2]))
        return out
