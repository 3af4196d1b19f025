"""The PPO rollout buffer on the device: SB3's `RolloutBuffer` and the bookkeeping of `OnPolicyAlgorithm.collect_rollouts` for a batch of envs
(training/config/algorithm/ppo.yaml: n_steps, gamma, gae_lambda), plus the episode sums `Monitor` and callbacks/logging_callback.py keep on the host.

The on-policy counterpart of `her.HerBuffer`: a step's rows go into the buffer without leaving the device, returns and advantages are computed there, and
`get()` yields minibatches of device tensors (csrc/hrgym_rollout.h: kernels, layout, arithmetic).  The flat order of everything gathered or exported is SB3's
swap_and_flatten: i = env * n_steps + step.

    env = HipVecEnv(4096)
    env.attach_rollout(n_steps=64, gamma=0.99, gae_lambda=0.9)
    env.collect_rollout(policy, value_fn)          # n_steps steps, nothing leaves the device
    for batch in env.rollout.get(batch_size=4096): # RolloutBufferSamples of device tensors
        ...
    env.rollout.episode_stats()                    # dict(episodes, r, l, collision, n_goal_reached, ...): sums over the finished episodes
"""
import ctypes
from collections import namedtuple

import numpy as np

from ._cstruct import CONST, RolloutDesc
from ._device import EpisodeBuffer, check_columns
from ._lib import _ptr

# the fields SB3's PPO.train reads (stable_baselines3.common.type_aliases.RolloutBufferSamples)
RolloutBufferSamples = namedtuple("RolloutBufferSamples", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns"])

STATS_DIM = 3 + CONST["HRG_INFO_DIM"]   # episodes, return, length, the info columns
# the arrays of hrg_rollout_export behind the state word, in its order
_EXPORT_KEYS = ("observations", "actions", "rewards", "values", "log_probs", "episode_starts", "advantages", "returns", "cur_obs", "flags", "run_return", "run_length", "stats")


def build_rollout_desc(n_envs, n_steps, obs_cols, act_dim=CONST["HRG_ACT_DIM"], gamma=0.99, gae_lambda=0.95):
    """hrg_rollout_desc (include/hrgym.h).  `obs_cols`: the column of the observation superset behind each value of the policy's observation."""
    n_envs, n_steps, act_dim, gamma, gae_lambda = int(n_envs), int(n_steps), int(act_dim), float(gamma), float(gae_lambda)
    if n_envs < 1 or n_steps < 1:
        raise ValueError(f"rollout: n_envs = {n_envs} and n_steps = {n_steps} must be positive")
    if not (0.0 <= gamma <= 1.0 and 0.0 <= gae_lambda <= 1.0):
        raise ValueError(f"rollout: gamma = {gamma} and gae_lambda = {gae_lambda} must lie in [0, 1]")
    cols = check_columns("rollout", obs_cols, act_dim)
    d = RolloutDesc()
    d.n_envs, d.n_steps, d.gamma, d.gae_lambda, d.act_dim, d.n_obs_cols = n_envs, n_steps, gamma, gae_lambda, act_dim, len(cols)
    for k, c in enumerate(cols):
        d.obs_cols[k] = c
    return d


# ---- the index arithmetic of the grouped minibatches (RolloutBuffer.get_groups), on tensors of any device
def group_rows(n_envs, n_steps, n_groups, batch_size):
    """(n_groups, the m * n_steps rows of a group) for `n_envs` envs in `n_groups` groups of m consecutive envs; NotImplementedError for groups that do not
    divide the envs and for a batch_size that does not divide a group's rows (the learner takes no short last minibatch)."""
    n, T, P, B = int(n_envs), int(n_steps), int(n_groups), int(batch_size)
    if P < 1 or n % P:
        raise NotImplementedError(f"n_envs = {n} is not divisible by n_groups = {P}: every member reads a group of the same size")
    rows = n // P * T
    if B < 1 or rows % B:
        raise NotImplementedError(f"batch_size = {B} does not divide m * n_steps = {rows} (m = {n // P} envs per group): the learner takes no short last minibatch")
    return P, rows


def group_table(perms, rows):
    """The permutations of 0 .. rows - 1, one per group, as the int64 [n_groups, rows] table of flat indices: group p's moved by p * rows."""
    import torch
    table = torch.stack(list(perms))
    return table + rows * torch.arange(table.shape[0], dtype=table.dtype, device=table.device)[:, None]


def group_batch(table, k0, batch_size):
    """Minibatch k0 / batch_size of every group, one behind the other: cat_p(table[p, k0:k0 + batch_size]), int64 [n_groups * batch_size]."""
    return table[:, k0:k0 + batch_size].reshape(-1)


class RolloutBuffer(EpisodeBuffer):
    """A device-resident rollout buffer of `desc.n_steps` slots for each of `desc.n_envs` envs (hrg_rollout_desc; `build_rollout_desc`).  All arguments and
    results are torch tensors on the buffer's device; the calls are asynchronous, ordered on torch's current stream (`episode_stats` and `export`
    synchronise).  `info_keys`: names of the info block's columns, for `episode_stats`.  `seed`: of the generator `get` draws its permutations with."""

    _prefix = "hrg_rollout"

    def __init__(self, desc, device=0, info_keys=None, seed=0):
        self._open(desc, device, info_keys)
        torch = self.torch
        self.n, self.n_steps, self.act_dim, self.obs_dim = int(desc.n_envs), int(desc.n_steps), int(desc.act_dim), int(desc.n_obs_cols)
        self.gamma, self.gae_lambda = float(desc.gamma), float(desc.gae_lambda)
        with torch.cuda.device(self.device):
            self.generator = torch.Generator(device=self.device)
            self.generator.manual_seed(int(seed))
        self.pos = 0               # slots written since the last reset()
        self.last_indices = None   # the permutation (or the caller's indices) behind the last get()

    @property
    def full(self):
        return self.pos == self.n_steps

    def _per_env(self, x, what):
        """A float32 value per env: [n] or [n, 1] (a value head's output), contiguous."""
        if x.dim() == 2 and x.shape[1] == 1:
            x = x.reshape(-1)
        return x, self._tensor(x, self.torch.float32, (self.n,), what)

    def view(self, rows, out=None):
        """The policy's view of rows of the observation superset: float32 [m, 64] -> float32 [m, n_obs_cols] (value k = column obs_cols[k])."""
        return self._view(rows, None, out)

    def observe(self, obs, mask=None):
        """The rows an episode starts from, after a reset: `obs` float32 [n, 64]; `mask` uint8 [n] (None: every env).  A masked env's next slot is an
        episode start, and its running return and length start again."""
        self._observe(obs, None, mask)

    def add_step(self, actions, values, log_probs, terminal_values, obs, term_obs, reward, done, info):
        """One slot per env, from the policy's outputs and the tensors a step wrote: `actions` float32 [n, act_dim] as the policy emitted them (not
        clipped), `values`, `log_probs` float32 [n]; `terminal_values` float32 [n] or None: the value of `view(term_obs)`, added to the reward (times
        gamma) where the step was truncated by the time limit; `obs` float32 [n, 64] (after auto-reset), `reward` float32 [n], `done` uint8 [n], `info`
        int32 [n, HRG_INFO_DIM].  `term_obs` (float32 [n, 64] or None) is what `terminal_values` was evaluated on; the buffer does not read it."""
        t, C = self.torch, CONST
        values, pv = self._per_env(values, "values")
        log_probs, pl = self._per_env(log_probs, "log_probs")
        ptv = None
        if terminal_values is not None:
            terminal_values, ptv = self._per_env(terminal_values, "terminal_values")
        if term_obs is not None:
            self._tensor(term_obs, t.float32, (self.n, C["HRG_OBS_DIM"]), "term_obs")
        args = (self._tensor(actions, t.float32, (self.n, self.act_dim), "actions"), pv, pl, ptv, self._tensor(obs, t.float32, (self.n, C["HRG_OBS_DIM"]), "obs"),
                self._tensor(reward, t.float32, (self.n,), "reward"), self._tensor(done, t.uint8, (self.n,), "done"),
                self._tensor(info, t.int32, (self.n, C["HRG_INFO_DIM"]), "info"))
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_rollout_add(self.h, *args, self._stream()))
        self.pos += 1

    def compute_returns_and_advantage(self, last_values):
        """GAE(lambda) over the full buffer (SB3's compute_returns_and_advantage; `dones` are the buffer's own flags): `last_values` float32 [n], the
        value of `observation()` after the last step."""
        last_values, p = self._per_env(last_values, "last_values")
        with self.torch.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_rollout_compute(self.h, p, self._stream()))

    def _gather(self, idx):
        t = self.torch
        B = int(idx.shape[0])
        new = lambda *shape: t.empty(*shape, dtype=t.float32, device=self.device)   # noqa: E731
        out = (new(B, self.obs_dim), new(B, self.act_dim), new(B), new(B), new(B), new(B))
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_rollout_get(self.h, _ptr(idx), B, *map(_ptr, out), self._stream()))
        return RolloutBufferSamples(*out)

    def get(self, batch_size=None, generator=None, indices=None):
        """Minibatches of the full, computed buffer (SB3's get): yields RolloutBufferSamples of `batch_size` samples (None: all n_envs * n_steps in one)
        that together cover one `torch.randperm` of the flat range, drawn on the device with `generator` (default: the buffer's own); the last batch is
        short when batch_size does not divide.  `indices`: int64 flat indices on the device instead (repeats allowed; checked against the range, which
        reads their extremes back), yielded as one batch."""
        t = self.torch
        N = self.n * self.n_steps
        if indices is not None:
            if batch_size is not None:
                raise ValueError("get: batch_size or indices, not both")
            if indices.dtype != t.int64 or indices.device != self.device or indices.dim() != 1 or not indices.is_contiguous() or indices.numel() < 1:
                raise ValueError(f"indices: expected a non-empty contiguous int64 vector on {self.device}, got {indices.dtype} {tuple(indices.shape)} on {indices.device}")
            lo, hi = int(indices.min()), int(indices.max())
            if lo < 0 or hi >= N:
                raise IndexError(f"indices: {lo} .. {hi} outside the flat range 0 .. {N - 1} (index = env * n_steps + step)")
            self.last_indices = indices
            yield self._gather(indices)
            return
        B = N if batch_size is None else int(batch_size)
        if B < 1:
            raise ValueError("get: batch_size must be positive")
        with t.cuda.device(self.device):
            perm = t.randperm(N, device=self.device, generator=self.generator if generator is None else generator)
        self.last_indices = perm
        for k0 in range(0, N, B):
            yield self._gather(perm[k0:k0 + B])

    def get_groups(self, n_groups, batch_size, seeds=None):
        """`get` for a population (ppo.PpoPopulation): the envs are `n_groups` groups of m = n_envs / n_groups consecutive envs, group p the flat range
        [p m n_steps, (p + 1) m n_steps).  Yields RolloutBufferSamples of n_groups * batch_size samples, group p's rows at p * batch_size, that cover one
        `torch.randperm(m * n_steps)` per group, drawn on the device with a generator of the group's own, seeded `seeds[p]` (default: p) -- what `get` of a
        lone buffer of the group's m envs with that seed draws.  The generators are made on first use and kept; another seeds list reseeds them.  Each
        minibatch is one gather; `last_indices` is the int64 [n_groups, m * n_steps] table of the epoch."""
        t = self.torch
        P, rows = group_rows(self.n, self.n_steps, n_groups, batch_size)
        seeds = [int(s) & 0xFFFFFFFFFFFFFFFF for s in (range(P) if seeds is None else seeds)]
        if len(seeds) != P:
            raise ValueError(f"get_groups: {len(seeds)} seeds for {P} groups")
        with t.cuda.device(self.device):
            if getattr(self, "_group_seeds", None) != seeds:
                self._group_generators = [t.Generator(device=self.device) for _ in seeds]
                for g, s in zip(self._group_generators, seeds):
                    g.manual_seed(s)
                self._group_seeds = seeds
            table = group_table([t.randperm(rows, device=self.device, generator=g) for g in self._group_generators], rows)
        self.last_indices = table
        return (self._gather(group_batch(table, k0, int(batch_size))) for k0 in range(0, rows, int(batch_size)))   # (the refusals above come with the call)

    def reset(self):
        """SB3's rollout_buffer.reset(): the position back to 0.  Current rows, flags, running returns and episode accumulators stay."""
        self._check(self.lib, self.lib.hrg_rollout_reset(self.h))
        self.pos = 0

    def export(self):
        """Every array of the buffer on the host, in the flat order (synchronous; tests): dict of observations [N, n_obs_cols], actions [N, act_dim], rewards,
        values, log_probs, episode_starts, advantages, returns [N], cur_obs [n, 64], flags [n], run_return, run_length [n], stats [n, 3 + HRG_INFO_DIM],
        pos, computed."""
        n, N = self.n, self.n * self.n_steps
        f32 = lambda *s: np.zeros(s, np.float32)   # noqa: E731
        arrays = (f32(N, self.obs_dim), f32(N, self.act_dim), f32(N), f32(N), f32(N), f32(N), f32(N), f32(N), f32(n, CONST["HRG_OBS_DIM"]), f32(n),
                  np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros((n, STATS_DIM), np.float64))
        state = np.zeros(2, np.int64)
        self._check(self.lib, self.lib.hrg_rollout_export(self.h, *(a.ctypes.data_as(ctypes.c_void_p) for a in arrays + (state,))))
        out = dict(zip(_EXPORT_KEYS, arrays))
        out.update(pos=int(state[0]), computed=bool(state[1]))
        return out
