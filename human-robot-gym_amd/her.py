"""Hindsight experience replay on the device: the replay buffer of SAC + HER (training/config/algorithm/sac_her.yaml) for a batch of goal envs.

The reference trains with SB3's `HerReplayBuffer`, patched by wrappers/HER_buffer_add_monkey_patch.py, and refuses more than one env
(utils/training_utils_SB3.py:154).  Here every env of a `HipVecEnv(goal_env=True)` has a ring of transitions in device memory; the step's rows go into
it without leaving the device, and `sample()` returns device tensors (csrc/hrgym_her.h: kernels, ring rules and the sampling rule).

    env = HipVecEnv(4096, goal_env=True)
    env.attach_her(buffer_size=256)            # transitions per env
    ...                                        # reset() / step() fill env.her
    batch = env.her.sample(256)                # DictReplayBufferSamples of device tensors

and, for the device learner (sac.SacLearner), the same samples as the rows a MultiInputPolicy feeds its MLPs, with nothing read back:

    learner = env.attach_sac(batch_size=128)   # obs_dim = env.her.obs_features
    env.collect_steps(learner.act, 100)        # env.her.observation() is the policy's input
    learner.train(env.her, 400)                # 400 x (env.her.sample_features(128), step)
    env.her.episode_stats()                    # dict(episodes, r, l, collision, n_goal_reached, ...): sums over the finished episodes
"""
import ctypes
from collections import namedtuple

import numpy as np

from ._cstruct import CONST, HerDesc
from ._device import EpisodeBuffer, check_columns
from ._lib import _ptr
from .replay import ReplayBufferSamples

# the fields SB3's SAC reads (stable_baselines3.common.type_aliases.DictReplayBufferSamples); observations / next_observations are dicts
DictReplayBufferSamples = namedtuple("DictReplayBufferSamples", ["observations", "actions", "next_observations", "dones", "rewards"])

STRATEGIES = {"future": CONST["HRG_HER_FUTURE"], "final": CONST["HRG_HER_FINAL"], "episode": CONST["HRG_HER_EPISODE"]}
GOAL_KINDS = {"reach": CONST["HRG_GOAL_REACH"], "cube": CONST["HRG_GOAL_CUBE"]}
AG_DIM = {CONST["HRG_GOAL_REACH"]: 6, CONST["HRG_GOAL_CUBE"]: 7}
DG_DIM = {CONST["HRG_GOAL_REACH"]: 6, CONST["HRG_GOAL_CUBE"]: 3}
FEATURE_KEYS = ("achieved_goal", "desired_goal", "observation")   # gym.spaces.Dict orders its keys alphabetically; CombinedExtractor concatenates in that order


def feature_slices(goal_kind, n_obs_cols):
    """Where each entry of the dict observation sits in the feature row a MultiInputPolicy feeds its MLPs (SB3 1.5.0's CombinedExtractor over Box entries
    [UPSTREAM]: flatten and concatenate in the Dict space's key order): dict name -> slice, in that order.  `goal_kind`: "reach" / "cube" or HRG_GOAL_*."""
    kind = GOAL_KINDS[goal_kind] if isinstance(goal_kind, str) else int(goal_kind)
    out, o = {}, 0
    for key, w in zip(FEATURE_KEYS, (AG_DIM[kind], DG_DIM[kind], int(n_obs_cols))):
        out[key] = slice(o, o + w)
        o += w
    return out


def her_ratio(n_sampled_goal):
    """Share of the samples that are relabelled (HerReplayBuffer.__init__)."""
    return 1.0 - 1.0 / (1.0 + int(n_sampled_goal))


def build_her_desc(n_envs, capacity, horizon, goal_kind, obs_cols, act_dim=CONST["HRG_ACT_DIM"], model_desc=None, n_sampled_goal=4, goal_selection_strategy="future",
                   ratio=None, seed=0, act_low=None, act_high=None, dg_in_obs=(), relabel_observation=False, **reward):
    """hrg_her_desc (include/hrgym.h).  The reward / done parameters come from `model_desc` (an hrg_model_desc), overridden by keywords (goal_dist,
    task_reward, object_gripped_reward, reward_shaping, collision_reward, reward_scale, done_at_success, done_at_collision).  `act_low` / `act_high`:
    the action bounds, given when the stored actions are to be rescaled to [-1, 1].  `ratio`: her_ratio itself, instead of n_sampled_goal."""
    if goal_selection_strategy not in STRATEGIES:
        raise ValueError(f"goal_selection_strategy {goal_selection_strategy!r}: one of {sorted(STRATEGIES)}")
    d = HerDesc()
    d.n_envs, d.capacity, d.horizon = int(n_envs), int(capacity), int(horizon)
    d.goal_kind = GOAL_KINDS[goal_kind] if isinstance(goal_kind, str) else int(goal_kind)
    d.strategy = STRATEGIES[goal_selection_strategy]
    d.her_ratio = her_ratio(n_sampled_goal) if ratio is None else float(ratio)
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    fields = ("goal_dist", "task_reward", "object_gripped_reward", "reward_shaping", "collision_reward", "reward_scale", "done_at_success", "done_at_collision")
    unknown = sorted(set(reward) - set(fields))
    if unknown:
        raise TypeError(f"build_her_desc: unexpected arguments {unknown}")
    for k in fields:
        if k in reward:
            setattr(d, k, type(getattr(d, k))(reward[k]))
        elif model_desc is not None:
            setattr(d, k, getattr(model_desc, k))
    d.act_dim = int(act_dim)
    d.rescale_actions = int(act_low is not None)
    if act_low is not None:
        for k in range(d.act_dim):
            d.act_low[k], d.act_high[k] = float(act_low[k]), float(act_high[k])
    cols = check_columns("her", obs_cols, ranges=False)   # (columns outside the superset and act_dim: hrg_her_create's refusals)
    d.n_obs_cols = len(cols)
    for k, c in enumerate(cols):
        d.obs_cols[k] = c
    d.relabel_observation = int(bool(relabel_observation))
    d.n_dg_in_obs = len(dg_in_obs)
    for k, c in enumerate(dg_in_obs):
        d.dg_in_obs[k] = int(c)
    return d


class HerBuffer(EpisodeBuffer):
    """A device-resident hindsight replay buffer of `desc.n_envs` rings (hrg_her_desc; `build_her_desc`).  All arguments and results are torch tensors on
    the buffer's device; the calls are asynchronous, ordered on torch's current stream (`sample` waits for the prefix sum's total; `sample_features` and
    `observation` wait for nothing; `episode_stats`, `counts_host` and `export` synchronise).  `info_keys`: names of the info block's columns, for
    `episode_stats`."""

    _prefix = "hrg_her"

    def __init__(self, desc, device=0, info_keys=None):
        self._open(desc, device, info_keys)
        self.n, self.capacity, self.act_dim, self.obs_dim = int(desc.n_envs), int(desc.capacity), int(desc.act_dim), int(desc.n_obs_cols)
        self.ag_dim, self.dg_dim = AG_DIM.get(desc.goal_kind, 0), DG_DIM.get(desc.goal_kind, 0)
        self.obs_features = self.ag_dim + self.dg_dim + self.obs_dim   # F: the width of the feature row achieved_goal | desired_goal | observation
        self._cum = None   # the exclusive prefix sums of `counts` sample_features draws from, until observe / add_step change the counts
        with self.torch.cuda.device(self.device):
            self.counts = self.torch.zeros(self.n, dtype=self.torch.int64, device=self.device)   # closed transitions per env, written by the add / observe kernels
        self.record_index = False   # tests: keep the (env, counter, goal counter) rows of the last sample() in `last_index`
        self.last_index = None

    def observe(self, obs, mask=None):
        """The rows an episode starts from, after a reset: `obs` float32 [n, 64]; `mask` uint8 [n] (None: every env).  The unfinished episode of a masked
        env is discarded."""
        t = self.torch
        o = self._tensor(obs, t.float32, (self.n, CONST["HRG_OBS_DIM"]), "obs")
        m = None if mask is None else self._tensor(mask, t.uint8, (self.n,), "mask")
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_her_observe(self.h, o, m, _ptr(self.counts), self._stream()))
        self._cum = None

    def add_step(self, actions, obs, term_obs, reward, done, info):
        """One transition per env, from the tensors a step wrote: `actions` float64 [n, 7] as the step left them, `obs` / `term_obs` float32 [n, 64], `reward`
        float32 [n], `done` uint8 [n], `info` int32 [n, HRG_INFO_DIM]."""
        t, C = self.torch, CONST
        args = (self._tensor(actions, t.float64, (self.n, C["HRG_ACT_DIM"]), "actions"), self._tensor(obs, t.float32, (self.n, C["HRG_OBS_DIM"]), "obs"),
                self._tensor(term_obs, t.float32, (self.n, C["HRG_OBS_DIM"]), "term_obs"), self._tensor(reward, t.float32, (self.n,), "reward"),
                self._tensor(done, t.uint8, (self.n,), "done"), self._tensor(info, t.int32, (self.n, C["HRG_INFO_DIM"]), "info"))
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_her_add(self.h, *args, _ptr(self.counts), self._stream()))
        self._cum = None

    def add(self, *args, **kwargs):
        """Nothing: the transition went into the buffer on the device when the env stepped.  Lets the object stand where an off-policy loop expects a
        replay buffer."""

    def sample(self, batch_size, env=None):
        """`batch_size` transitions, uniform over the finished episodes' transitions of all envs, a share `her_ratio` of them relabelled.  `env` (SB3 passes
        its VecNormalize) is not used."""
        t = self.torch
        B = int(batch_size)
        if B < 1:
            raise ValueError("sample: batch_size must be positive")
        with t.cuda.device(self.device):
            cum = t.zeros(self.n + 1, dtype=t.int64, device=self.device)
            t.cumsum(self.counts, 0, out=cum[1:])
            new = lambda w: t.empty(B, w, dtype=t.float32, device=self.device)   # noqa: E731
            obs, ag, dg, nobs, nag, ndg = new(self.obs_dim), new(self.ag_dim), new(self.dg_dim), new(self.obs_dim), new(self.ag_dim), new(self.dg_dim)
            act, rew, done = new(self.act_dim), new(1), new(1)
            idx = t.empty(B, CONST["HRG_HER_INDEX_DIM"], dtype=t.int64, device=self.device) if self.record_index else None
            self._check(self.lib, self.lib.hrg_her_sample(self.h, B, *map(_ptr, (cum, obs, ag, dg, nobs, nag, ndg, act, rew, done, idx)), self._stream()))
        self.last_index = idx
        return DictReplayBufferSamples(observations=dict(observation=obs, achieved_goal=ag, desired_goal=dg), actions=act,
                                       next_observations=dict(observation=nobs, achieved_goal=nag, desired_goal=ndg), dones=done, rewards=rew)

    def feature_slices(self):
        """dict name -> slice of the feature row, in SB3's key order: achieved_goal, desired_goal, observation (`feature_slices`)."""
        return feature_slices(self.desc.goal_kind, self.obs_dim)

    def _check_features(self):
        if self.obs_features > CONST["HRG_OBS_DIM"]:
            raise NotImplementedError(f"her: a feature row of {self.ag_dim} + {self.dg_dim} + {self.obs_dim} values (achieved_goal, desired_goal, observation): the "
                                      f"kernels keep one value per lane, at most {CONST['HRG_OBS_DIM']}; select fewer observation columns (obs_keys)")

    def observation(self, rows=None):
        """The feature row of every env's current row (SB3's _last_obs as a MultiInputPolicy sees it): float32 [n, obs_features]; with `rows` float32
        [m, 64], of those rows of the observation superset: float32 [m, obs_features]."""
        t = self.torch
        self._check_features()
        m = self.n if rows is None else int(rows.shape[0]) if rows.dim() == 2 else -1
        r = None if rows is None else self._tensor(rows, t.float32, (m, CONST["HRG_OBS_DIM"]), "rows")
        out = t.empty(m, self.obs_features, dtype=t.float32, device=self.device)
        self._call("features", r, m, _ptr(out))
        return out

    def sample_features(self, batch_size):
        """The samples of `sample` -- the same draws and the same call counter -- as feature rows: ReplayBufferSamples(observations [B, obs_features], actions
        [B, act_dim], next_observations [B, obs_features], dones [B, 1], rewards [B, 1]).  Nothing is read back and nothing synchronises: whether the buffer
        holds a finished episode is the caller's check (`size()`, once before a run of calls; on an empty buffer the tensors come back unwritten)."""
        t = self.torch
        B = int(batch_size)
        if B < 1:
            raise ValueError("sample_features: batch_size must be positive")
        self._check_features()
        with t.cuda.device(self.device):
            if self._cum is None:
                self._cum = t.zeros(self.n + 1, dtype=t.int64, device=self.device)
                t.cumsum(self.counts, 0, out=self._cum[1:])
            new = lambda w: t.empty(B, w, dtype=t.float32, device=self.device)   # noqa: E731
            feat, nfeat, act, rew, done = new(self.obs_features), new(self.obs_features), new(self.act_dim), new(1), new(1)
            idx = t.empty(B, CONST["HRG_HER_INDEX_DIM"], dtype=t.int64, device=self.device) if self.record_index else None
            self._check(self.lib, self.lib.hrg_her_sample_features(self.h, B, *map(_ptr, (self._cum, feat, nfeat, act, rew, done, idx)), self._stream()))
        self.last_index = idx
        return ReplayBufferSamples(observations=feat, actions=act, next_observations=nfeat, dones=done, rewards=rew)

    def require_samples(self):
        """Raises unless an episode has finished (synchronous): the check `sample` makes on every call, for a caller of `sample_features`."""
        if self.size() < 1:
            raise ValueError("her: no finished episode in the buffer yet (nothing to sample)")

    def compute_reward_done(self, achieved_goal, desired_goal, collision_type):
        """HipVecEnv.compute_reward / compute_done of device rows (hrg_goal_reward_done): float32 [n, ag_dim], float32 [n, dg_dim], int32 [n] ->
        (reward float32 [n], done bool [n])."""
        t = self.torch
        n = int(achieved_goal.shape[0])
        args = (self._tensor(achieved_goal, t.float32, (n, self.ag_dim), "achieved_goal"), self._tensor(desired_goal, t.float32, (n, self.dg_dim), "desired_goal"),
                self._tensor(collision_type, t.int32, (n,), "collision_type"))
        reward, done = t.empty(n, dtype=t.float32, device=self.device), t.empty(n, dtype=t.uint8, device=self.device)
        with t.cuda.device(self.device):   # (the entry point launches on the current device)
            self._check(self.lib, self.lib.hrg_goal_reward_done(ctypes.byref(self.desc), *args, n, _ptr(reward), _ptr(done), self._stream()))
        return reward, done.bool()

    def counts_host(self):
        """(transitions stored, transitions of finished episodes, sample calls so far); synchronous."""
        c = (ctypes.c_int64 * 3)()
        self._check(self.lib, self.lib.hrg_her_counts(self.h, c))
        return tuple(int(x) for x in c)

    def size(self):
        """Transitions that can be sampled (synchronous)."""
        return self.counts_host()[1]

    def export(self, env):
        """Env's whole ring on the host (synchronous; tests): dict of pre, post [cap, 64], action [cap, act_dim], reward, done, truncated, collision_type,
        ep_start, ep_len [cap], w, tail, open, cur_obs [64]."""
        cap, od = self.capacity, CONST["HRG_OBS_DIM"]
        out = dict(pre=np.zeros((cap, od), np.float32), post=np.zeros((cap, od), np.float32), action=np.zeros((cap, self.act_dim), np.float32),
                   reward=np.zeros(cap, np.float32), done=np.zeros(cap, np.uint8), truncated=np.zeros(cap, np.uint8), collision_type=np.zeros(cap, np.int32),
                   ep_start=np.zeros(cap, np.int64), ep_len=np.zeros(cap, np.int32), state=np.zeros(3, np.int64), cur_obs=np.zeros(od, np.float32))
        self._check(self.lib, self.lib.hrg_her_export(self.h, int(env), *(a.ctypes.data_as(ctypes.c_void_p) for a in out.values())))
        st = out.pop("state")
        out.update(w=int(st[0]), tail=int(st[1]), open=int(st[2]))
        return out
