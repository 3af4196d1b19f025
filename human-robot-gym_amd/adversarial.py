"""Adversarial imitation on the device (Ho & Ermon 2016, GAIL; Fu, Luo, Levine 2018, AIRL; off-policy as in Kostrikov et al. 2019): the imitation reward
that needs neither the live scripted expert (the action imitation reward) nor a time-aligned demonstration and a per-task distance (the state imitation
reward).  A discriminator D(obs, action) is trained to tell the rows of a demonstration table (bc.DemoTable, dagger.DaggerTable) from the learner's own rows,
and SAC's batch is relabelled with the current discriminator at sample time:

    r = r_disc alpha + r_env (1 - alpha),    r_disc = -log(1 - D) = softplus(d)  (reward="gail")  |  logit D = d  (reward="airl")

The discriminator is an MLP of a SAC critic's shape on [obs | action] with one output, the logit d that the row is the expert's.  One update is two kernel
launches with no vendor BLAS and no autograd (csrc/hrgym_disc.h: the launches, the draws, the loss), the reward is one forward launch.

    env = HipVecEnv(1024, env_id="ReachHuman", obs_norm=...)
    env.attach_replay(buffer_size=1_000_000)
    learner = env.attach_sac(batch_size=128)
    disc = env.attach_discriminator("reach-demo", batch_size=128)     # a dataset name, path, ExpertDataset, or a table of env.demonstrations(...)
    env.collect_steps(learner.act, 100)
    adversarial.train_sac(learner, env.replay, disc, 400, alpha=0.25)  # 400 x (sample, discriminator step, reward, SAC step); nothing synchronises
    disc.diagnostics()                                                 # loss, expert_accuracy, policy_accuracy of the last update (synchronous)

Out of scope: PPO, populations, goal envs, absorbing states, gradient penalty, state-only discriminators."""
import ctypes
import math

import numpy as np

from ._cstruct import CONST, DiscDesc
from ._device import DeviceHandle
from ._learner import LearnerParams, build_layout, check_widths, mlp_entries
from ._lib import _ptr

HIDDEN = CONST["HRG_SAC_HIDDEN"]
MAX_DEPTH = CONST["HRG_SAC_MAX_DEPTH"]
TILE = CONST["HRG_SAC_TILE"]
MAX_BATCH = CONST["HRG_DISC_MAX_BATCH"]
ACTIVATIONS = {"relu": CONST["HRG_DISC_RELU"], "tanh": CONST["HRG_DISC_TANH"]}
REWARDS = {"gail": CONST["HRG_DISC_REWARD_GAIL"], "airl": CONST["HRG_DISC_REWARD_AIRL"]}


def param_layout(obs_dim, act_dim, depth):
    """The discriminator's flat parameter vector (csrc/hrgym_disc.h): (OrderedDict name -> (offset, shape), n_params) under the names of a torch Sequential,
    disc.{0, 2, ..}.weight / .bias for the hidden layers and disc.{2 depth}.* for the head."""
    return build_layout([*mlp_entries("disc", depth, int(obs_dim) + int(act_dim), HIDDEN), (f"disc.{2 * depth}.weight", (1, HIDDEN)), (f"disc.{2 * depth}.bias", (1,))])


def check_alpha(alpha):
    if not 0.0 <= float(alpha) <= 1.0:   # (a NaN fails both comparisons)
        raise ValueError(f"discriminator: alpha = {alpha} outside [0, 1]: the weight of the discriminator's reward against the env's")
    return float(alpha)


def check_learning_rate(learning_rate):
    if not math.isfinite(float(learning_rate)) or float(learning_rate) < 0.0:
        raise ValueError(f"discriminator: learning_rate = {learning_rate}: a finite learning rate that is not negative")
    return float(learning_rate)


def build_disc_desc(obs_dim, act_dim, net_arch=(64, 64), activation="relu", batch_size=128, reward="gail", seed=0):
    """hrg_disc_desc (include/hrgym.h).  Everything the kernels do not cover is refused here, before anything is allocated or launched."""
    arch = [int(w) for w in net_arch]
    if not 1 <= len(arch) <= MAX_DEPTH or any(w != HIDDEN for w in arch):
        raise NotImplementedError(f"discriminator: net_arch = {arch}: the kernels cover hidden width {HIDDEN} and depth 1 .. {MAX_DEPTH}")
    if activation not in ACTIVATIONS:
        raise ValueError(f"discriminator: activation = {activation!r}: one of {sorted(ACTIVATIONS)}")
    if reward not in REWARDS:
        raise ValueError(f"discriminator: reward = {reward!r}: one of {sorted(REWARDS)}")
    obs_dim, act_dim, batch_size = check_widths(obs_dim, act_dim, batch_size, TILE, MAX_BATCH)
    d = DiscDesc()
    d.obs_dim, d.act_dim, d.depth, d.hidden, d.batch_size = obs_dim, act_dim, len(arch), HIDDEN, batch_size
    d.activation, d.reward_kind, d.seed = ACTIVATIONS[activation], REWARDS[reward], int(seed) & 0xFFFFFFFFFFFFFFFF
    return d


def check_table(table):
    """The refusals of what is no table of a SAC learner's demonstrations, before anything is allocated."""
    kind = getattr(table, "kind", None)
    if kind not in ("sac", "ppo"):
        raise ValueError(f"discriminator: {type(table).__name__} is no table of demonstrations (env.demonstrations(dataset))")
    if kind != "sac":
        raise ValueError(f"discriminator: a table of kind {kind!r}: the discriminator compares the table's actions with the replay buffer's, which are at the "
                         "policy's scale [-1, 1]; a 'ppo' table holds them at the env's (build the table with the replay buffer attached)")
    return table


class Discriminator(DeviceHandle):
    """The discriminator of `table` (a bc.DemoTable or dagger.DaggerTable of kind "sac"; its `n_rows` is read at every step) against rows of the same widths.
    `p`: its tensors (LearnerParams: `params`, `adam_m`, `adam_v` float32 [n_params], initialised with torch.nn.Linear's default under `seed`), the handle's
    own.  `learning_rate` is a plain attribute, passed with every step: a caller may schedule it.  `step`, `reward` and `logits` are asynchronous, ordered on
    torch's current stream; `diagnostics` and `export` synchronise."""
    _create, _destroy = "hrg_disc_create", "hrg_disc_destroy"

    def __init__(self, table, net_arch=(64, 64), activation="relu", batch_size=128, learning_rate=3e-4, reward="gail", seed=0):
        check_table(table)
        desc = build_disc_desc(table.obs_dim, table.act_dim, net_arch=net_arch, activation=activation, batch_size=batch_size, reward=reward, seed=seed)
        learning_rate = check_learning_rate(learning_rate)
        self._open(desc, table.device.index)
        self.table, self.obs_dim, self.act_dim, self.depth, self.batch_size = table, int(desc.obs_dim), int(desc.act_dim), int(desc.depth), int(desc.batch_size)
        self.activation, self.reward_kind, self.learning_rate = activation, reward, learning_rate
        layout, n_params = param_layout(self.obs_dim, self.act_dim, self.depth)
        self.p = LearnerParams(layout, n_params, seed, self.device)
        if self._sizes()[0] != n_params:
            raise RuntimeError(f"Discriminator: the library lays out {self._sizes()[0]} parameters, adversarial.param_layout {n_params}: rebuild")
        self._keep = None

    def _sizes(self):
        w = (ctypes.c_int64 * 4)()
        self._check(self.lib, self.lib.hrg_disc_sizes(self.h, w))
        return [int(x) for x in w]

    @property
    def n_updates(self):
        """Updates so far: the count behind Adam's bias corrections and the draws' key."""
        return self._sizes()[1]

    def _rows(self, obs, actions):
        t = self.torch
        if obs.dim() != 2:
            raise ValueError(f"obs: expected [n, {self.obs_dim}], got {tuple(obs.shape)}")
        n = int(obs.shape[0])
        if n < 1:
            raise ValueError("discriminator: n = 0 rows: a call takes at least one")
        return n, self._tensor(obs, t.float32, (n, self.obs_dim), "obs"), self._tensor(actions, t.float32, (n, self.act_dim), "actions")

    def step(self, obs, actions, indices=None):
        """One update: `batch_size` rows of the table -- drawn by the handle, or `indices` int64 [batch_size] on the device (tests; IndexError for a row
        outside the table, which reads their extremes back) -- against the learner's rows `obs` float32 [batch_size, obs_dim], `actions` float32
        [batch_size, act_dim]."""
        t, tb, B, p = self.torch, self.table, self.batch_size, self.p
        if tb.n_rows == 0:   # (a dagger.DaggerTable without pinned rows, before its first step)
            raise ValueError("discriminator: the table is empty (n_rows = 0): a step draws its expert rows from the table")
        lr = check_learning_rate(self.learning_rate)
        o, a = self._tensor(obs, t.float32, (B, self.obs_dim), "obs"), self._tensor(actions, t.float32, (B, self.act_dim), "actions")
        pi = None
        if indices is not None:
            pi = self._tensor(indices, t.int64, (B,), "indices")
            lo, hi = int(indices.min()), int(indices.max())
            if lo < 0 or hi >= tb.n_rows:
                raise IndexError(f"indices: rows {lo} .. {hi} outside the table's {tb.n_rows} rows")
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_disc_step(self.h, _ptr(tb.observations), _ptr(tb.actions), tb.n_rows, pi, o, a, _ptr(p.params), _ptr(p.adam_m), _ptr(p.adam_v),
                                                          lr, self._stream()))
        self._keep = (obs, actions, indices)

    def _column(self, x, n, what):
        """A value per row, float32 [n] or [n, 1], or None."""
        if x is None:
            return None
        return self._tensor(x, self.torch.float32, (n,) if x.dim() == 1 else (n, 1), what)

    def _forward(self, obs, actions, env_rewards, alpha, out, logits):
        n, o, a = self._rows(obs, actions)
        r, w, lg = self._column(env_rewards, n, "env_rewards"), self._column(out, n, "out"), self._column(logits, n, "logits")
        with self.torch.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_disc_reward(self.h, _ptr(self.p.params), o, a, n, r, float(alpha), w, lg, self._stream()))

    def reward(self, obs, actions, env_rewards=None, alpha=1.0, out=None):
        """The reward of the rows `obs` float32 [n, obs_dim], `actions` float32 [n, act_dim], n >= 1: r_disc = softplus(d) ("gail") or d ("airl"); with
        `env_rewards` float32 [n] or [n, 1], r_disc alpha + r_env (1 - alpha).  `out` float32 [n] or [n, 1]: written in place (it may be `env_rewards` itself)
        and returned; without it a new tensor of `env_rewards`' shape, or [n].  Nothing of the discriminator moves."""
        alpha = check_alpha(alpha)
        if out is None:
            out = self.torch.empty_like(env_rewards) if env_rewards is not None else self.torch.empty(int(obs.shape[0]) if obs.dim() == 2 else 0, dtype=self.torch.float32, device=self.device)
        self._forward(obs, actions, env_rewards, alpha, out, None)
        return out

    def logits(self, obs, actions):
        """The logits d float32 [n] of the rows: positive where the discriminator takes a row for the expert's.  Nothing of the discriminator moves."""
        out = self.torch.empty(int(obs.shape[0]) if obs.dim() == 2 else 0, dtype=self.torch.float32, device=self.device)
        self._forward(obs, actions, None, 1.0, None, out)
        return out

    def export(self):
        """The last step's intermediates on the host (synchronous; tests): indices int64 [B] (the table rows), logits float32 [2 B] (expert rows, then policy
        rows), grad float32 [n_params] in the parameters' layout, loss, expert_accuracy, policy_accuracy."""
        B = self.batch_size
        idx, logits, grad, diag = np.zeros(B, np.int64), np.zeros(2 * B, np.float32), np.zeros(self.p.n_params, np.float32), np.zeros(3, np.float32)
        self._check(self.lib, self.lib.hrg_disc_export(self.h, *(a.ctypes.data_as(ctypes.c_void_p) for a in (idx, logits, grad, diag))))
        return dict(indices=idx, logits=logits, grad=grad, loss=float(diag[0]), expert_accuracy=float(diag[1]), policy_accuracy=float(diag[2]))

    def diagnostics(self):
        """dict(loss: the last update's binary cross-entropy; expert_accuracy, policy_accuracy: the shares of its expert rows with d > 0 and of its policy
        rows with d < 0; n_updates; learning_rate).  Synchronous."""
        diag = np.zeros(3, np.float32)
        self._check(self.lib, self.lib.hrg_disc_export(self.h, None, None, None, diag.ctypes.data_as(ctypes.c_void_p)))
        return dict(loss=float(diag[0]), expert_accuracy=float(diag[1]), policy_accuracy=float(diag[2]), n_updates=self.n_updates, learning_rate=self.learning_rate)

    def state_dict(self):
        """Copies on the host of the parameters, Adam's moments (float32 [n_params]) and the step count: what `load_state_dict` continues bit for bit from."""
        return dict(params=self.p.params.detach().cpu().clone(), adam_m=self.p.adam_m.detach().cpu().clone(), adam_v=self.p.adam_v.detach().cpu().clone(),
                    n_updates=self.n_updates)

    def load_state_dict(self, state):
        t = self.torch
        for name in ("params", "adam_m", "adam_v"):
            src, own = t.as_tensor(state[name]), getattr(self.p, name)
            if tuple(src.shape) != tuple(own.shape):
                raise ValueError(f"load_state_dict: {name} has shape {tuple(src.shape)}, expected {tuple(own.shape)} (a discriminator of other shapes)")
            with t.no_grad():
                own.copy_(src.to(device=own.device, dtype=own.dtype))
        self._check(self.lib, self.lib.hrg_disc_restore(self.h, int(state["n_updates"])))


def train_sac(learner, replay, disc, gradient_steps, disc_every=1, alpha=1.0):
    """SAC on the discriminator's reward: `gradient_steps` x (replay.sample(batch_size); every `disc_every`-th step (0: never) a discriminator update on the
    batch's rows against the table's; the batch's rewards rewritten in place to r_disc alpha + r_env (1 - alpha) with the current discriminator;
    learner.step(batch)), with no copy to the host and no synchronisation.  With disc_every = 0 and alpha = 0 it is learner.train(replay, gradient_steps)."""
    if int(getattr(learner, "n_members", 1)) != 1 or hasattr(replay, "sample_features"):
        raise NotImplementedError("train_sac: adversarial imitation covers a lone sac.SacLearner on a replay.ReplayBuffer (no population, no hindsight buffer)")
    if disc.batch_size != learner.batch_size:
        raise ValueError(f"train_sac: the discriminator's batch_size = {disc.batch_size}, the learner's = {learner.batch_size}: a step reads one batch for both")
    if (disc.obs_dim, disc.act_dim) != (learner.obs_dim, learner.act_dim):
        raise ValueError(f"train_sac: the discriminator takes observations of {disc.obs_dim} and actions of {disc.act_dim} values, the learner {learner.obs_dim} and {learner.act_dim}")
    learner._check_buffer(replay.obs_dim, replay.act_dim)
    alpha, every = check_alpha(alpha), int(disc_every)
    for i in range(int(gradient_steps)):
        batch = replay.sample(learner.batch_size)
        if every > 0 and i % every == 0:
            disc.step(batch.observations, batch.actions)
        disc.reward(batch.observations, batch.actions, env_rewards=batch.rewards, alpha=alpha, out=batch.rewards)
        learner.step(batch)
