"""DAgger on the device (Ross, Gordon, Bagnell 2011): the states the learner's own policy reaches, labelled by the live scripted expert, aggregated into a table
that bc.BehaviourCloning trains on.  A table of a recorded dataset (bc.DemoTable) holds only states the expert visited; once the clone drifts off them nothing
corrects it.  Here every env step labels the row the learner was just shown with the expert's action for it, draws per env whether the expert or the learner
drives the step (the expert with probability `beta`), and writes the (view, label) pair into the table -- one kernel launch between the learner's action and
the step kernel (csrc/hrgym_dagger.h), nothing leaves the device.

    env = HipVecEnv(1024, env_id="ReachHuman", expert=dict(id="ReachHuman", signal_to_noise_ratio=1.0), obs_norm=...)
    env.attach_replay(buffer_size=1_000_000)
    learner = env.attach_sac(batch_size=128)
    dagger = env.attach_dagger(capacity=200_000, beta=0.5, table=env.demonstrations("reach-demo"))   # the dataset's rows: iteration 0, never overwritten
    bc = env.attach_bc(dagger.table, batch_size=128)
    for i in range(10):
        dagger.beta = 0.5 * 0.7 ** i
        env.collect_dagger(100)        # 100 x (observation, learner.act, expert, the dagger step, the env step, replay.add_step); nothing synchronises
        bc.train(500)
        dagger.stats()                 # steps, the share the expert drove, the on-policy imitation error (synchronous)

With beta = 1 the same loop fills SAC's replay buffer with the expert's transitions, rewards included: something for the critics to fit before fine-tuning
(`learner.train(env.replay, k)`).

What differs from the textbook: the aggregate is a ring of `capacity_steps` step slots behind the pinned rows (the oldest step is overwritten; the textbook keeps
everything), and the mixture is drawn per env and step (the textbook's beta_i mixes per query too, but is often implemented per episode).  Every step calls the
expert once, which advances its Ornstein-Uhlenbeck noise once: clean labels need the expert's signal_to_noise_ratio = 1."""
import ctypes

import numpy as np

from ._cstruct import CONST, DaggerDesc
from ._device import DeviceHandle
from ._lib import _ptr
from .bc import DemoTable

KINDS = {"sac": CONST["HRG_BC_SAC"], "ppo": CONST["HRG_BC_PPO"]}   # the table's kind -> hrg_dagger_desc.kind
STATS_DIM = CONST["HRG_DAGGER_STATS_DIM"]


class DaggerTable(DemoTable):
    """The growing table: `observations` float32 [pinned_rows + capacity_steps * n_envs, K] and `actions` float32 [.., A], allocated once.  The first
    `pinned_rows` rows are a copy of `pinned` (a bc.DemoTable of the same kind and widths: DAgger's iteration 0) and are never overwritten; behind them step slot
    s holds the n_envs rows of one step, env e at row pinned_rows + s * n_envs + e; the slot wraps.  `n_rows`: the rows written so far, what
    BehaviourCloning draws from -- 0 for a table without pinned rows until the first step.  `kind` is the learner's ("sac": actions at the policy's scale)."""

    def __init__(self, torch, kind, n_envs, obs_dim, act_dim, capacity_steps, device, pinned=None):
        if kind not in KINDS:
            raise ValueError(f"DaggerTable: kind = {kind!r}: 'sac' or 'ppo'")
        self.kind, self.n_envs, self.obs_dim, self.act_dim, self.capacity_steps = kind, int(n_envs), int(obs_dim), int(act_dim), int(capacity_steps)
        self.pinned_rows, self.device = 0 if pinned is None else int(pinned.n_rows), device
        self.steps = 0   # steps written, as the handle counts them (Dagger.step)
        rows = self.pinned_rows + self.capacity_steps * self.n_envs
        self.observations = torch.zeros(rows, self.obs_dim, dtype=torch.float32, device=device)
        self.actions = torch.zeros(rows, self.act_dim, dtype=torch.float32, device=device)
        if pinned is not None:
            self.observations[:self.pinned_rows] = pinned.observations
            self.actions[:self.pinned_rows] = pinned.actions

    @property
    def n_rows(self):
        return self.pinned_rows + min(self.steps, self.capacity_steps) * self.n_envs


def check_dagger(kind, n_envs, obs_dim, act_dim, capacity_steps, low, high, beta, pinned, device):
    """What hrg_dagger_create refuses, and a pinned table that does not fit, before anything is allocated; returns the bounds as float64 arrays."""
    if kind not in KINDS:
        raise ValueError(f"dagger: kind = {kind!r}: 'sac' or 'ppo'")
    if int(n_envs) < 1:
        raise ValueError(f"dagger: n_envs = {n_envs} must be positive")
    if not 1 <= int(obs_dim) <= CONST["HRG_OBS_DIM"]:
        raise NotImplementedError(f"dagger: obs_dim = {obs_dim} outside 1 .. {CONST['HRG_OBS_DIM']} (the kernel moves one value of the view per lane)")
    if not 1 <= int(act_dim) <= CONST["HRG_ACT_DIM"]:
        raise NotImplementedError(f"dagger: act_dim = {act_dim} outside 1 .. {CONST['HRG_ACT_DIM']}")
    if int(capacity_steps) < 1:
        raise ValueError(f"dagger: capacity_steps = {capacity_steps} must be positive")
    low, high = np.asarray(low, np.float64).reshape(-1), np.asarray(high, np.float64).reshape(-1)
    if low.shape != (int(act_dim),) or high.shape != (int(act_dim),):
        raise ValueError(f"dagger: bounds of {low.shape[0]} and {high.shape[0]} values for actions of {act_dim}")
    if not (np.isfinite(low).all() and np.isfinite(high).all() and (high > low).all()):
        raise ValueError(f"dagger: the action bounds must be finite with high > low, got low = {low.tolist()}, high = {high.tolist()}")
    check_beta(beta)
    if pinned is not None:
        if getattr(pinned, "kind", None) != kind:
            raise ValueError(f"dagger: a pinned table of kind {getattr(pinned, 'kind', None)!r} for a {kind} learner: SAC's actions are stored at the policy's scale [-1, 1], "
                             "PPO's at the env's (build the table with the learner's buffer attached)")
        if (pinned.obs_dim, pinned.act_dim) != (int(obs_dim), int(act_dim)):
            raise ValueError(f"dagger: the pinned table holds observations of {pinned.obs_dim} and actions of {pinned.act_dim} values, the steps write {obs_dim} and {act_dim}")
        if device is not None and pinned.device != device:
            raise ValueError(f"dagger: the pinned table lives on {pinned.device}, the envs on {device}")
    return low, high


def check_beta(beta):
    if not 0.0 <= float(beta) <= 1.0:   # (a NaN fails both comparisons)
        raise ValueError(f"dagger: beta = {beta} outside [0, 1]: the probability that the expert drives an env's step")
    return float(beta)


class Dagger(DeviceHandle):
    """The DAgger step for `n_envs` envs with global ids `env_id0` .. and a learner of `kind` ("sac" | "ppo"), and the table it fills (`table`, a DaggerTable of
    `capacity_steps` step slots behind the rows of `pinned`).  `low`, `high`: the action space's bounds [act_dim].  `beta`: the probability that the expert drives
    an env's step, a plain attribute passed with every step: a caller may schedule it.  `n_calls`: steps so far, the key of the next step's draws.  `step` is
    asynchronous, ordered on torch's current stream; `stats` synchronises."""
    _create, _destroy = "hrg_dagger_create", "hrg_dagger_destroy"

    def __init__(self, kind, n_envs, obs_dim, act_dim, capacity_steps, low, high, beta=0.5, pinned=None, seed=0, env_id0=0, device=0):
        import torch
        dev = torch.device("cuda", device)
        low, high = check_dagger(kind, n_envs, obs_dim, act_dim, capacity_steps, low, high, beta, pinned, dev)
        desc = DaggerDesc()
        desc.kind, desc.n_envs, desc.env_id0, desc.obs_dim, desc.act_dim = KINDS[kind], int(n_envs), int(env_id0), int(obs_dim), int(act_dim)
        desc.capacity_steps, desc.pinned_rows, desc.seed = int(capacity_steps), 0 if pinned is None else int(pinned.n_rows), int(seed) & 0xFFFFFFFFFFFFFFFF
        for j in range(int(act_dim)):
            desc.act_low[j], desc.act_high[j] = float(low[j]), float(high[j])
        self._open(desc, device)
        self.n, self.obs_dim, self.act_dim, self.beta, self.n_calls = int(n_envs), int(obs_dim), int(act_dim), float(beta), 0
        with torch.cuda.device(self.device):
            self.table = DaggerTable(torch, kind, n_envs, obs_dim, act_dim, capacity_steps, self.device, pinned)

    def sizes(self):
        """dict(n_calls, slot, n_rows, bytes) as the handle keeps them: steps so far, the next step slot, the table's valid rows, device memory held."""
        w = (ctypes.c_int64 * 4)()
        self._check(self.lib, self.lib.hrg_dagger_sizes(self.h, w))
        return dict(zip(("n_calls", "slot", "n_rows", "bytes"), (int(x) for x in w)))

    def step(self, view, learner_actions, expert_actions, rows_out, kept_out=None):
        """One step.  `view` float32 [n, obs_dim]: the attached buffer's view of the current rows, what the learner was just shown; `learner_actions` float32
        [n, act_dim]: the learner's action (SAC: at the policy's scale; PPO: at the env's, not clipped); `expert_actions` float64 [n, HRG_ACT_DIM]: the batch's
        expert buffer.  Writes the table's rows of the slot, `rows_out` float64 [n, HRG_ACT_DIM] (what the step kernel reads: the clipped expert action where
        the expert drives, else the learner's action brought to the bounds; zeros behind act_dim) and `kept_out` float32 [n, act_dim] or None (the executed
        action at the policy's scale, for the replay buffer's add_step), and adds to the statistics."""
        t, tb, n, A = self.torch, self.table, self.n, self.act_dim
        beta = check_beta(self.beta)
        args = (self._tensor(view, t.float32, (n, self.obs_dim), "view"), self._tensor(learner_actions, t.float32, (n, A), "learner_actions"),
                self._tensor(expert_actions, t.float64, (n, CONST["HRG_ACT_DIM"]), "expert_actions"), beta, _ptr(tb.observations), _ptr(tb.actions),
                self._tensor(rows_out, t.float64, (n, CONST["HRG_ACT_DIM"]), "rows_out"),
                None if kept_out is None else self._tensor(kept_out, t.float32, (n, A), "kept_out"))
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_dagger_step(self.h, *args, self._stream()))
        self.n_calls += 1
        tb.steps = self.n_calls

    def stats_per_env(self, clear=True):
        """float64 [n, 3]: steps, steps the expert drove, the sum over the steps of sum_j (a_j - label_j)^2 (synchronous)."""
        acc = np.zeros((self.n, STATS_DIM), np.float64)
        self._check(self.lib, self.lib.hrg_dagger_stats(self.h, acc.ctypes.data_as(ctypes.c_void_p), int(bool(clear))))
        return acc

    def stats(self, clear=True):
        """The steps since the last clear, summed over the envs: dict(steps, expert_steps, sq_error -- the sums -- and the means expert_fraction =
        expert_steps / steps and imitation_error = sq_error / (steps * act_dim): the mean squared difference, over steps and components, between the learner's
        deterministic action at the label's scale and the label on the states the mixture visited -- behaviour cloning's loss, on policy; nan without steps),
        and n_rows, beta.  Synchronous."""
        return summarise(self.stats_per_env(clear).sum(axis=0), self.act_dim, n_rows=self.table.n_rows, beta=self.beta)


def summarise(tot, act_dim, **extra):
    steps, expert, sq = int(tot[CONST["HRG_DAGGER_STEPS"]]), int(tot[CONST["HRG_DAGGER_EXPERT_STEPS"]]), float(tot[CONST["HRG_DAGGER_SQ_ERROR"]])
    nan = float("nan")
    return dict(steps=steps, expert_steps=expert, sq_error=sq, expert_fraction=expert / steps if steps else nan,
                imitation_error=sq / (steps * int(act_dim)) if steps else nan, **extra)
