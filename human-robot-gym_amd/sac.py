"""The SAC gradient step on the device: SB3 1.5.0's `SAC.train` for `MlpPolicy` with hidden width 64 and `use_sde=False` (training/config_icra_2024/
.../*-SAC.yaml: net_arch [64, 64, 64], batch_size 128, ent_coef auto_0.2), next to the replay buffer it reads (replay.ReplayBuffer).

One gradient step is six kernel launches with no vendor BLAS and no autograd (csrc/hrgym_sac.h: the launches, the parameter layout, the draws, what differs
from SB3).  Parameters, Adam moments and target parameters are flat float32 torch tensors; `state_dict()` hands out views under SB3's parameter names.

    env = HipVecEnv(4096, env_id="ReachHuman", obs_norm=...)
    env.attach_replay(buffer_size=1_000_000)
    learner = env.attach_sac(batch_size=128, learning_rate=5e-4, ent_coef="auto_0.2", seed=0)
    env.collect_steps(learner.act, 100)            # train_freq steps with the learner's actor as the policy
    learner.train(env.replay, 400)                 # 400 x (sample, gradient step): nothing leaves the device, nothing synchronises
    learner.diagnostics()                          # ent_coef, actor_loss, critic_loss, ent_coef_loss of the last step (synchronous)

SAC + HER (training/config/algorithm/sac_her.yaml: policy MultiInputPolicy) runs on the same kernels.  SB3 1.5.0's MultiInputPolicy with its default
CombinedExtractor flattens the Box entries of the dict observation and concatenates them in the Dict space's (alphabetical) key order [UPSTREAM], so the MLPs
read the row achieved_goal | desired_goal | observation; her.HerBuffer hands out exactly that row (`observation`, `sample_features`):

    env = HipVecEnv(4096, goal_env=True, obs_keys=["object-state", "robot0_joint_pos", "robot0_joint_vel"])
    env.attach_her(buffer_size=256)
    learner = env.attach_sac(batch_size=128)       # policy="MultiInputPolicy", obs_dim = env.her.obs_features
    env.collect_steps(learner.act, 100)
    learner.train(env.her, 400)                    # 400 x (env.her.sample_features(128), step): one read of the buffer's size, then nothing synchronises
"""
import ctypes
import math

import numpy as np

from ._cstruct import CONST, SacDesc, SacHyper
from ._learner import (MAX_POPULATION, Learner, LearnerParams, Population, PopulationParams, build_layout, check_seeds, check_widths, mlp_entries,  # noqa: F401 (check_seeds: importable from here)
                       per_member, refuse_shared_sequences, scheduled_attribute)
from ._lib import _ptr

HIDDEN = CONST["HRG_SAC_HIDDEN"]
MAX_DEPTH = CONST["HRG_SAC_MAX_DEPTH"]
TILE = CONST["HRG_SAC_TILE"]
MAX_BATCH = CONST["HRG_SAC_MAX_BATCH"]
NQ = CONST["HRG_SAC_NQ"]
Q_COLUMNS = ("q1", "q2", "q1_target", "q2_target", "q1_pi", "q2_pi")   # the rows of hrg_sac_export's q, in its order


POLICIES = {False: "MlpPolicy", True: "MultiInputPolicy"}   # by goal_env: what SB3 takes for a Box and for a Dict observation space


def check_policy(policy, goal_env):
    """`policy` (None: the default) for an env with flat (`goal_env` False) or dict observations; the other policy is refused by name."""
    want = POLICIES[bool(goal_env)]
    if policy is None:
        return want
    if policy not in POLICIES.values():
        raise NotImplementedError(f"policy = {policy!r}: the device learner covers {sorted(POLICIES.values())}")
    if policy != want:
        raise NotImplementedError(f"policy = {policy!r}: {'a goal env has dict observations' if goal_env else 'this env has flat observations'}, which SB3 gives to {want}")
    return policy


def depth_of(net_arch):
    """Hidden layers of `net_arch`; NotImplementedError for what the kernels do not cover."""
    if isinstance(net_arch, dict):
        raise NotImplementedError(f"net_arch = {net_arch}: separate actor and critic architectures are not supported (a list of hidden widths)")
    arch = [int(w) for w in net_arch]
    if not 1 <= len(arch) <= MAX_DEPTH or any(w != HIDDEN for w in arch):
        raise NotImplementedError(f"net_arch = {arch}: the kernels cover hidden width {HIDDEN} and depth 1 .. {MAX_DEPTH} (the ICRA configs' [64, 64, 64])")
    return len(arch)


def parse_ent_coef(ent_coef):
    """SB3's ent_coef: "auto" (learned, from 1), "auto_<x>" (learned, from x) or a float (fixed) -> (learned, initial or fixed value)."""
    if isinstance(ent_coef, str):
        if not ent_coef.startswith("auto"):
            raise ValueError(f"ent_coef = {ent_coef!r}: 'auto', 'auto_<initial value>' or a float")
        init = float(ent_coef.split("_")[1]) if "_" in ent_coef else 1.0
        if not init > 0.0:
            raise ValueError("ent_coef: the initial value of the entropy coefficient must be greater than 0")
        return True, init
    value = float(ent_coef)
    if not value > 0.0 or not math.isfinite(value):
        raise ValueError(f"ent_coef = {ent_coef}: a fixed entropy coefficient must be positive and finite")
    return False, value


def build_sac_desc(obs_dim, act_dim, net_arch=(64, 64, 64), gamma=0.99, tau=0.005, ent_coef="auto", target_entropy="auto", batch_size=256,
                   target_update_interval=1, seed=0):
    """hrg_sac_desc (include/hrgym.h).  Everything the kernels do not cover is refused here, before anything is allocated or launched."""
    depth = depth_of(net_arch)
    obs_dim, act_dim, batch_size = check_widths(obs_dim, act_dim, batch_size, TILE, MAX_BATCH)
    if int(target_update_interval) < 1:
        raise ValueError(f"target_update_interval = {target_update_interval} must be positive")
    learned, value = parse_ent_coef(ent_coef)
    d = SacDesc()
    d.obs_dim, d.act_dim, d.depth, d.hidden, d.batch_size = obs_dim, act_dim, depth, HIDDEN, batch_size
    d.auto_ent_coef, d.target_update_interval = int(learned), int(target_update_interval)
    d.gamma, d.tau, d.ent_coef = float(gamma), float(tau), value
    d.target_entropy = -float(act_dim) if isinstance(target_entropy, str) and target_entropy == "auto" else float(target_entropy)   # -prod(action_space.shape)
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return d


def param_layout(obs_dim, act_dim, depth):
    """The flat parameter vector (csrc/hrgym_sac.h): OrderedDict name -> (offset, shape) under SB3 1.5.0's names ([UPSTREAM]: from knowledge of that release),
    actor | critic.qf0 | critic.qf1 | log_ent_coef, and (n_params, n_actor, n_critic).  The targets are the two critics' entries as `critic_target.*`, offsets
    less n_actor, in a vector of their own."""
    K, A, H = int(obs_dim), int(act_dim), HIDDEN
    entries = [*mlp_entries("actor.latent_pi", depth, K, H), ("actor.mu.weight", (A, H)), ("actor.log_std.weight", (A, H)), ("actor.mu.bias", (A,)),
               ("actor.log_std.bias", (A,))]
    for q in range(2):
        entries += [*mlp_entries(f"critic.qf{q}", depth, K + A, H), (f"critic.qf{q}.{2 * depth}.weight", (1, H)), (f"critic.qf{q}.{2 * depth}.bias", (1,))]
    out, n = build_layout(entries + [("log_ent_coef", (1,))])
    n_actor = out["critic.qf0.0.weight"][0]
    return out, (n, n_actor, (n - 1 - n_actor) // 2)


class SacParams(LearnerParams):
    """The learner's tensors, on any torch device: `params`, `adam_m`, `adam_v` float32 [n_params] and `target` float32 [2 n_critic], with `state_dict()`
    views under SB3's names.  Initial weights: torch.nn.Linear's own initialisation under a generator seeded with `seed` (actor, mu, log_std, qf0, qf1, in
    that order); the targets start as copies; log_ent_coef = log(`ent_coef_init`)."""

    def __init__(self, obs_dim, act_dim, depth, seed=0, ent_coef_init=1.0, device="cpu"):
        self.obs_dim, self.act_dim, self.depth, self.ent_coef_init = int(obs_dim), int(act_dim), int(depth), float(ent_coef_init)
        layout, (n_params, self.n_actor, self.n_critic) = param_layout(obs_dim, act_dim, depth)
        super().__init__(layout, n_params, seed, device)
        self.target = self.params[self.n_actor:self.n_actor + 2 * self.n_critic].clone()

    def _init_rest(self, flat):
        flat[-1] = math.log(self.ent_coef_init)

    def state_dict(self):
        """OrderedDict of views into `params` and `target` under SB3's names (writing into one writes the learner's parameter): actor.latent_pi.{0,2,4}.*,
        actor.mu.*, actor.log_std.*, critic.qf{0,1}.{0,2,4,6}.*, log_ent_coef, then critic_target.qf{0,1}.*.  The same names under MultiInputPolicy: its
        CombinedExtractor over Box entries is a Flatten per entry and has no parameters ([UPSTREAM]: from knowledge of SB3 1.5.0), so a dict-observation SAC
        holds the MLPs' entries only."""
        out = super().state_dict()
        for name, (off, shape) in self.layout.items():
            if name.startswith("critic."):
                o = off - self.n_actor
                out["critic_target." + name[len("critic."):]] = self.target[o:o + int(np.prod(shape))].view(shape)
        return out

    def group(self, flat, which):
        """The slice of a parameter-shaped vector that belongs to "actor", "qf0", "qf1" or "log_ent_coef"."""
        a, c = self.n_actor, self.n_critic
        lo, hi = dict(actor=(0, a), qf0=(a, a + c), qf1=(a + c, a + 2 * c), log_ent_coef=(a + 2 * c, a + 2 * c + 1))[which]
        return flat[lo:hi]


class SacLearner(Learner):
    """SB3's SAC on the device for the shapes the kernels cover (`build_sac_desc` refuses the rest).  `learning_rate` is a plain attribute, passed with every
    step: a caller may schedule it.  All tensor arguments and results live on the learner's device; `step`, `train` and `act` are asynchronous, ordered on
    torch's current stream; `diagnostics` and `export` synchronise."""

    _prefix = "hrg_sac"
    n_members = 1   # (SacPopulation: more)

    def __init__(self, obs_dim, act_dim, net_arch=(64, 64, 64), learning_rate=3e-4, gamma=0.99, tau=0.005, ent_coef="auto", target_entropy="auto",
                 batch_size=256, target_update_interval=1, seed=0, device=0):
        desc = build_sac_desc(obs_dim, act_dim, net_arch=net_arch, gamma=gamma, tau=tau, ent_coef=ent_coef, target_entropy=target_entropy, batch_size=batch_size,
                              target_update_interval=target_update_interval, seed=seed)
        self._open(desc, device)
        self.obs_dim, self.act_dim, self.depth, self.batch_size = int(obs_dim), int(act_dim), int(self.desc.depth), int(batch_size)
        self.learning_rate = float(learning_rate)
        self.auto_ent_coef = bool(self.desc.auto_ent_coef)
        self.p = SacParams(obs_dim, act_dim, self.depth, seed=seed, ent_coef_init=self.desc.ent_coef, device=self.device)
        sizes = self._sizes()
        if sizes[:3] != [self.p.n_params, self.p.n_actor, self.p.n_critic]:
            raise RuntimeError(f"SacLearner: the library lays out {sizes[:3]} parameters, sac.param_layout {[self.p.n_params, self.p.n_actor, self.p.n_critic]}: rebuild")
        self._keep = None

    def _hyper(self):
        return dict(learning_rate=self.learning_rate)

    @staticmethod
    def _checkpoint_kwargs(d, hyper):
        """The constructor's arguments, the seed apart, from a checkpoint's descriptor fields `d` and scheduled attributes `hyper`."""
        ent_coef = float(d["ent_coef"])
        return dict(obs_dim=int(d["obs_dim"]), act_dim=int(d["act_dim"]), net_arch=[int(d["hidden"])] * int(d["depth"]), learning_rate=float(hyper["learning_rate"]),
                    gamma=float(d["gamma"]), tau=float(d["tau"]), ent_coef=f"auto_{ent_coef!r}" if int(d["auto_ent_coef"]) else ent_coef,
                    target_entropy=float(d["target_entropy"]), batch_size=int(d["batch_size"]), target_update_interval=int(d["target_update_interval"]))

    @classmethod
    def _from_checkpoint(cls, d, hyper, device):
        """The learner of a checkpoint's descriptor fields `d` and scheduled attributes `hyper` (Learner.load)."""
        return cls(seed=int(d["seed"]), device=device, **cls._checkpoint_kwargs(d, hyper))

    def step(self, batch, eps_pi=None, eps_next=None):
        """One gradient step on `batch`, a ReplayBufferSamples of `batch_size` rows (observations, next_observations [B, obs_dim], actions [B, act_dim], dones,
        rewards [B, 1]).  `eps_pi` / `eps_next` float32 [B, act_dim]: the standard normal noise of the actor on the observations / the next observations, instead
        of the learner's own draws (tests).  A DictReplayBufferSamples (her.HerBuffer.sample) is accepted too: its entries are concatenated in the feature row's
        order (her.FEATURE_KEYS) first -- a convenience; `train` reads the buffer's feature rows directly.  A population takes its members' batches one behind
        the other, [P * B] rows."""
        B, K, A, p = self.n_members * self.batch_size, self.obs_dim, self.act_dim, self.p
        if isinstance(batch.observations, dict):
            from .her import FEATURE_KEYS
            from .replay import ReplayBufferSamples
            cat = lambda d: self.torch.cat([d[k] for k in FEATURE_KEYS], dim=1)   # noqa: E731
            batch = ReplayBufferSamples(cat(batch.observations), batch.actions, cat(batch.next_observations), batch.dones, batch.rewards)
        args = (self._tensor(batch.observations, (B, K), "observations"), self._tensor(batch.actions, (B, A), "actions"),
                self._tensor(batch.next_observations, (B, K), "next_observations"), self._tensor(batch.dones, (B, 1), "dones"),
                self._tensor(batch.rewards, (B, 1), "rewards"), None if eps_pi is None else self._tensor(eps_pi, (B, A), "eps_pi"),
                None if eps_next is None else self._tensor(eps_next, (B, A), "eps_next"))
        with self.torch.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_sac_step(self.h, *args, _ptr(p.params), _ptr(p.adam_m), _ptr(p.adam_v), _ptr(p.target), float(self._step_scalars()[0]), self._stream()))
        self._keep = (batch, eps_pi, eps_next)

    def _step_scalars(self):
        """(learning_rate,) as `step` passes it."""
        return (self.learning_rate,)

    def train(self, replay, gradient_steps):
        """SAC.train(gradient_steps, batch_size): `gradient_steps` x (replay.sample(batch_size), step), with no copy to the host and no synchronisation.
        `replay`: a replay.ReplayBuffer, or a her.HerBuffer, whose samples are its feature rows (`sample_features`): its size is read once, first (an empty
        hindsight buffer raises); after that line nothing on the host waits for the device."""
        hindsight = hasattr(replay, "sample_features")
        self._check_buffer(replay.obs_features if hindsight else replay.obs_dim, replay.act_dim)
        if hindsight:
            replay.require_samples()
        sample = replay.sample_features if hindsight else replay.sample
        for _ in range(int(gradient_steps)):
            self.step(sample(self.batch_size))

    def act(self, obs, deterministic=False, eps=None):
        """The actor's actions for `obs` float32 [n, obs_dim]: float32 [n, act_dim] in (-1, 1), tanh(mu + std eps), or tanh(mu) with `deterministic`.  This is the
        `policy` HipVecEnv.collect_steps takes.  `eps` float32 [n, act_dim] replaces the draws (tests)."""
        t = self.torch
        n, o, e = self._rows(obs, eps)
        out = t.empty(n, self.act_dim, dtype=t.float32, device=self.device)
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_sac_act(self.h, _ptr(self.p.params), o, n, e, int(bool(deterministic)), _ptr(out), self._stream()))
        return out

    def export(self, **which):
        """The last step's intermediates on the host (synchronous; tests): y, logp, logp_next [B]; q [6, B] (Q_COLUMNS); grad [n_params] in the parameters'
        layout (`self.p.group(grad, "actor")`, ...; the last entry is the coefficient's gradient); losses [4].  (`which`: SacPopulation's `member`.)"""
        B = self.batch_size
        y, logp, logp_next, q = (np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros((NQ, B), np.float32))
        grad, losses = np.zeros(self.p.n_params, np.float32), np.zeros(4, np.float32)
        self._export(y, logp, logp_next, q, grad, losses, **which)
        return dict(y=y, logp=logp, logp_next=logp_next, q=q, grad=grad, losses=losses)

    def diagnostics(self, **which):
        """What SB3 logs under train/ after a call of train(): ent_coef (the one the last step used), actor_loss, critic_loss, ent_coef_loss of the last step, and
        n_updates.  Synchronous."""
        losses = np.zeros(4, np.float32)
        self._export(None, None, None, None, None, losses, **which)
        return dict(ent_coef=float(losses[3]), actor_loss=float(losses[0]), critic_loss=float(losses[1]), ent_coef_loss=float(losses[2]), n_updates=self.n_updates)


class SacPopulationParams(PopulationParams):
    """The tensors of a population, on any torch device: `params`, `adam_m`, `adam_v` float32 [P, n_params] and `target` float32 [P, 2 n_critic].  Row p is
    initialised exactly as SacParams(seed=seeds[p], ent_coef_init=ent_coef_init[p]) (`ent_coef_init`: a scalar, or one value per member); `member(p)` is the
    rows of member p as views."""

    def __init__(self, obs_dim, act_dim, depth, seeds, ent_coef_init=1.0, device="cpu"):
        inits = per_member("ent_coef_init", ent_coef_init, len(seeds))
        rows = [SacParams(obs_dim, act_dim, depth, seed=int(s), ent_coef_init=e) for s, e in zip(seeds, inits)]
        super().__init__(rows, device)
        self.n_actor, self.n_critic = rows[0].n_actor, rows[0].n_critic


class SacPopulation(Population, SacLearner):
    """`n_members` SAC learners of the same shapes (SacLearner's keywords) that take their gradient step in the same six launches (csrc/hrgym_sac.h; DESIGN.md
    D27, D30): the seeds of one cell of a study, or the cells of a sweep, side by side on one GPU.  The batch of n = P m envs is P groups of m consecutive
    envs; member p acts in, and learns from, group p only.  The counters are shared: members step in lockstep.  `learning_rate`, `gamma`, `tau`, `ent_coef` and
    `target_entropy` take a scalar (every member) or a sequence of one value per member ("auto_0.2" next to a fixed 0.1 included); `learning_rate` may be
    assigned between steps, a scalar or a sequence.  What shapes a launch or the lockstep is shared (`_shared`).  Member p is, bit for bit,
    SacLearner(seed=seeds[p], **member_hyper(p)) on the same transitions.  export(member), diagnostics (a list of P dicts), member(p), member_hyper(p), save and
    load (member_<p>.npz and, where the members differ, population.npz): _learner.Population.

        env.attach_replay(buffer_size)
        pop = env.attach_sac_population(5, batch_size=128)       # seeds: the env's seed + p
        env.collect_steps(pop.act, 100)
        pop.train(env.replay, 800)                               # 800 x (env.replay.sample_groups(5, 128, pop.seeds), step)
        pop.diagnostics()                                        # a list of 5 dicts

        pop = env.attach_sac_population(6, seeds=[0, 1, 2] * 2, learning_rate=[1e-3] * 3 + [3e-4] * 3)   # a sweep: two learning rates x three seeds
    """
    _lone = SacLearner
    _fields = ("learning_rate", "gamma", "tau", "ent_coef", "target_entropy")
    _scheduled = ("learning_rate",)
    learning_rate = scheduled_attribute("learning_rate")
    _manifest_fields = ("learning_rate", "gamma", "tau", "ent_coef", "auto_ent_coef", "target_entropy")   # (the checkpoint's names: ent_coef is two descriptor fields)
    _shared = dict(net_arch="the depth shapes every launch", batch_size="the batch shapes every launch",
                   target_update_interval="the host decides per step whether the targets move, for all members of the lockstep")

    def __init__(self, obs_dim, act_dim, n_members, seeds, net_arch=(64, 64, 64), learning_rate=3e-4, gamma=0.99, tau=0.005, ent_coef="auto", target_entropy="auto",
                 batch_size=256, target_update_interval=1, device=0):
        self.n_members, table = check_seeds(n_members, seeds)
        self.seeds = [int(s) for s in table]
        self._kwargs = dict(net_arch=net_arch, batch_size=batch_size, target_update_interval=target_update_interval)   # (member, save and load: _learner.Population)
        refuse_shared_sequences(self._shared, self._kwargs)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self._set_values(learning_rate=learning_rate, gamma=gamma, tau=tau, ent_coef=ent_coef, target_entropy=target_entropy)
        descs = [self._member_desc(p) for p in range(self.n_members)]   # (every member's values are checked before anything is allocated)
        self._open(descs[0], device, self.n_members, table.ctypes.data_as(ctypes.c_void_p), create="_population_create")   # (the entry reads the table, not the descriptor's seed)
        self.depth, self.batch_size = int(self.desc.depth), int(batch_size)
        self.auto_ent_coef = bool(self.desc.auto_ent_coef)   # (member 0's; per member: member_hyper)
        self.p = SacPopulationParams(obs_dim, act_dim, self.depth, self.seeds, ent_coef_init=[d.ent_coef for d in descs], device=self.device)
        if self._sizes()[:3] != [self.p.n_params, self.p.n_actor, self.p.n_critic]:
            raise RuntimeError("SacPopulation: the library lays out other parameters than sac.param_layout: rebuild")
        self._keep = None
        self._sync_table()

    @staticmethod
    def _convert(name, value):
        """One member's value of a table field as the constructor takes it; ValueError for what no learner takes."""
        if name == "ent_coef":
            parse_ent_coef(value)
            return value if isinstance(value, str) else float(value)
        if name == "target_entropy" and isinstance(value, str):
            if value != "auto":
                raise ValueError(f"target_entropy = {value!r}: 'auto' or a float")
            return value
        value = float(value)
        if not math.isfinite(value) or (name == "learning_rate" and value < 0.0) or (name in ("gamma", "tau") and not 0.0 <= value <= 1.0):
            raise ValueError(f"{name} = {value}: " + ("a finite learning rate that is not negative" if name == "learning_rate" else "finite" if name == "target_entropy" else "in [0, 1]"))
        return value

    def _step_scalars(self):
        """Member 0's, kept as a tuple: the library reads its table once that is the caller's."""
        return self._member0

    def _member_desc(self, p):
        """Member p's descriptor: the lone learner's of its seed and its values."""
        v = self.member_hyper(p)
        return build_sac_desc(self.obs_dim, self.act_dim, seed=self.seeds[p], gamma=v["gamma"], tau=v["tau"], ent_coef=v["ent_coef"], target_entropy=v["target_entropy"],
                              **self._kwargs)

    def _row(self, p):
        d, row = self._member_desc(p), SacHyper()
        row.learning_rate, row.gamma, row.tau, row.ent_coef, row.target_entropy, row.auto_ent_coef = self._values["learning_rate"][p], d.gamma, d.tau, d.ent_coef, d.target_entropy, d.auto_ent_coef
        return row

    def train(self, replay, gradient_steps):
        """`gradient_steps` x (replay.sample_groups(n_members, batch_size, seeds), step), with no copy to the host and no synchronisation.  `replay`: a
        replay.ReplayBuffer over n_members groups of envs."""
        if not hasattr(replay, "sample_groups"):
            raise NotImplementedError(f"train: {type(replay).__name__} has no grouped sample (a population reads a replay.ReplayBuffer)")
        self._check_buffer(replay.obs_dim, replay.act_dim)
        for _ in range(int(gradient_steps)):
            self.step(replay.sample_groups(self.n_members, self.batch_size, self.seeds))

    def act(self, obs, deterministic=False, eps=None):
        """SacLearner.act for `obs` float32 [P m, obs_dim]: member p's actor on the rows of group p.  The `policy` HipVecEnv.collect_steps takes."""
        t = self.torch
        n, o, e = self._rows(obs, eps)
        if n % self.n_members:
            raise ValueError(f"act: {n} rows are not {self.n_members} groups of the same size")
        out = t.empty(n, self.act_dim, dtype=t.float32, device=self.device)
        with t.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_sac_population_act(self.h, _ptr(self.p.params), o, n // self.n_members, e, int(bool(deterministic)), _ptr(out), self._stream()))
        return out
