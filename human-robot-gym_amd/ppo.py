"""The PPO update on the device: SB3 1.5.0's `PPO.train` and `ActorCriticPolicy` for `MlpPolicy`, `use_sde=False` and Box actions, with tanh layers of width 64
(training/config/human_reach_ppo_parallel.yaml with algorithm/ppo.yaml: net_arch [64, 64], batch_size 64, n_epochs 20, log_std_init -2.7), next to the rollout
buffer it reads (rollout.RolloutBuffer).

One minibatch step is four kernel launches with no vendor BLAS and no autograd (csrc/hrgym_ppo.h: the launches, the parameter layout, the draws).  Parameters
and Adam moments are flat float32 torch tensors; `state_dict()` hands out views under SB3's parameter names.

    env = HipVecEnv(4096)
    env.attach_rollout(n_steps=64, gamma=0.99, gae_lambda=0.9)
    learner = env.attach_ppo(batch_size=64, n_epochs=20, learning_rate=7e-5, net_arch=[64, 64], log_std_init=-2.7, ortho_init=False)
    env.collect_rollout(learner.policy, learner.value)   # the learner supplies both callables
    learner.train(env.rollout)                           # n_epochs x (rollout.get(batch_size) -> step): no host copy, no synchronisation
    learner.diagnostics()                                # SB3's train/ keys of the last minibatch (synchronous)

The seeds of one cell of a study train side by side as a population (PpoPopulation): one set of launches per minibatch step for all of them.

    pop = env.attach_ppo_population(5, batch_size=64, n_epochs=20)   # 5 groups of num_envs / 5 envs; seeds: the env's seed + p
    env.collect_rollout(pop.policy, pop.value)
    pop.train(env.rollout)                                            # n_epochs x (rollout.get_groups(5, batch_size, pop.seeds) -> step)
"""
import ctypes
import math

import numpy as np

from ._cstruct import CONST, PpoDesc, PpoHyper
from ._learner import (MAX_POPULATION, Learner, LearnerParams, Population, PopulationParams, build_layout, check_seeds, check_widths, mlp_entries,  # noqa: F401 (MAX_POPULATION: importable from here)
                       refuse_shared_sequences, scheduled_attribute)
from ._lib import _ptr

HIDDEN = CONST["HRG_PPO_HIDDEN"]
MAX_DEPTH = CONST["HRG_PPO_MAX_DEPTH"]
TILE = CONST["HRG_PPO_TILE"]
MAX_BATCH = CONST["HRG_PPO_MAX_BATCH"]
NDIAG = CONST["HRG_PPO_NDIAG"]
DIAG_KEYS = ("policy_gradient_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "std", "grad_norm")   # hrg_ppo_export's diag, in its order
IGNORED_POLICY_KWARGS = ("full_std", "use_expln", "squash_output")   # [UPSTREAM] in 1.5.0 they reach gSDE and predict() only: no effect while use_sde is false
GROUPS = ("trunk", "action_net", "value_net", "log_std")


def parse_net_arch(net_arch):
    """SB3 1.5.0's net_arch of an ActorCriticPolicy -> (depth, separate).  [UPSTREAM] integers are shared layers, a trailing dict(pi=[...], vf=[...]) gives
    separate ones.  Two forms are covered, [64] * d (a shared trunk) and [dict(pi=[64] * d, vf=[64] * d)] (separate trunks), d = 1 .. 3; NotImplementedError
    for every other."""
    what = f"net_arch = {net_arch}"
    cover = f"the kernels cover [{HIDDEN}] * d (a shared trunk) and [dict(pi=[{HIDDEN}] * d, vf=[{HIDDEN}] * d)] (separate trunks), d = 1 .. {MAX_DEPTH}"
    if isinstance(net_arch, dict) or not isinstance(net_arch, (list, tuple)) or len(net_arch) == 0:
        raise NotImplementedError(f"{what}: {cover}")
    arch = list(net_arch)
    if isinstance(arch[-1], dict):
        if len(arch) > 1:
            raise NotImplementedError(f"{what}: shared layers under separate ones (a mixed arrangement) are not supported; {cover}")
        unknown = sorted(set(arch[0]) - {"pi", "vf"})
        if unknown:
            raise NotImplementedError(f"{what}: unknown keys {unknown}; {cover}")
        pi, vf = list(arch[0].get("pi", [])), list(arch[0].get("vf", []))
        if len(pi) != len(vf):
            raise NotImplementedError(f"{what}: unequal depths of pi and vf are not supported; {cover}")
        layers, separate = pi + vf, True
        depth = len(pi)
    else:
        if any(isinstance(w, dict) for w in arch):
            raise NotImplementedError(f"{what}: a dict is the last entry of net_arch; {cover}")
        layers, separate, depth = arch, False, len(arch)
    if any(int(w) != HIDDEN for w in layers):
        raise NotImplementedError(f"{what}: widths other than {HIDDEN} are not supported; {cover}")
    if not 1 <= depth <= MAX_DEPTH:
        raise NotImplementedError(f"{what}: depth {depth} outside 1 .. {MAX_DEPTH}; {cover}")
    return depth, separate


def build_ppo_desc(obs_dim, act_dim, net_arch=None, batch_size=64, rollout_size=0, normalize_advantage=True, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                   use_sde=False, target_kl=None, policy="MlpPolicy", seed=0):
    """hrg_ppo_desc (include/hrgym.h).  Everything the kernels do not cover is refused here, before anything is allocated or launched.  `net_arch` None: SB3's
    default [dict(pi=[64, 64], vf=[64, 64])].  `rollout_size`: n_envs * n_steps of the buffer the minibatches come from (0: not known)."""
    if use_sde:
        raise NotImplementedError("use_sde = True: state dependent exploration is not covered by the device learner")
    if target_kl is not None:
        raise NotImplementedError(f"target_kl = {target_kl}: the early stop needs a host readback per minibatch; the device learner runs every epoch (target_kl = None)")
    if policy != "MlpPolicy":
        raise NotImplementedError(f"policy = {policy!r}: the device learner covers MlpPolicy (dict observations belong to the off-policy path)")
    depth, separate = parse_net_arch([dict(pi=[64, 64], vf=[64, 64])] if net_arch is None else net_arch)
    (obs_dim, act_dim, batch_size), rollout_size = check_widths(obs_dim, act_dim, batch_size, TILE, MAX_BATCH), int(rollout_size)
    if rollout_size < 0 or rollout_size % batch_size:
        raise NotImplementedError(f"batch_size = {batch_size} does not divide n_envs * n_steps = {rollout_size}: the learner takes no short last minibatch")
    ent_coef, vf_coef, max_grad_norm = float(ent_coef), float(vf_coef), float(max_grad_norm)
    if not (math.isfinite(ent_coef) and math.isfinite(vf_coef) and ent_coef >= 0.0 and vf_coef >= 0.0):
        raise ValueError(f"ent_coef = {ent_coef} and vf_coef = {vf_coef} must be finite and not negative")
    if not (math.isfinite(max_grad_norm) and max_grad_norm > 0.0):
        raise ValueError(f"max_grad_norm = {max_grad_norm} must be finite and positive")
    d = PpoDesc()
    d.obs_dim, d.act_dim, d.depth, d.hidden, d.separate, d.batch_size, d.rollout_size = obs_dim, act_dim, depth, HIDDEN, int(separate), batch_size, rollout_size
    d.normalize_advantage, d.policy, d.use_sde, d.target_kl_set = int(bool(normalize_advantage)), CONST["HRG_PPO_MLP_POLICY"], 0, 0
    d.ent_coef, d.vf_coef, d.max_grad_norm = ent_coef, vf_coef, max_grad_norm
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return d


def param_layout(obs_dim, act_dim, depth, separate):
    """The flat parameter vector (csrc/hrgym_ppo.h): OrderedDict name -> (offset, shape) under SB3 1.5.0's names ([UPSTREAM]: from knowledge of that release):
    mlp_extractor.shared_net.{0,2,4}.* or mlp_extractor.policy_net.* | mlp_extractor.value_net.*, then action_net.weight, value_net.weight, action_net.bias,
    value_net.bias (the two heads are one [A + 1][64] product), then log_std."""
    K, A, H = int(obs_dim), int(act_dim), HIDDEN
    entries = [e for net in (("policy_net", "value_net") if separate else ("shared_net",)) for e in mlp_entries(f"mlp_extractor.{net}", depth, K, H)]
    return build_layout(entries + [("action_net.weight", (A, H)), ("value_net.weight", (1, H)), ("action_net.bias", (A,)), ("value_net.bias", (1,)), ("log_std", (A,))])


def group_of(name):
    """The parameter group of an entry of `param_layout`: "trunk", "action_net", "value_net" or "log_std"."""
    return "trunk" if name.startswith("mlp_extractor.") else name.split(".")[0]


class PpoParams(LearnerParams):
    """The learner's tensors, on any torch device: `params`, `adam_m`, `adam_v` float32 [n_params], with `state_dict()` views under SB3's names (log_std,
    mlp_extractor.shared_net.{0,2,4}.* or mlp_extractor.policy_net.* / mlp_extractor.value_net.*, action_net.*, value_net.*).  Initial weights are drawn under a
    forked generator seeded with `seed`, a layer after the other in the layout's order.  [UPSTREAM] `ortho_init` True: ActorCriticPolicy's orthogonal_ with gain
    sqrt 2 for the hidden layers, 0.01 for action_net and 1 for value_net, biases zero; False: torch.nn.Linear's own initialisation.  log_std = `log_std_init`
    in every component."""

    def __init__(self, obs_dim, act_dim, depth, separate, seed=0, log_std_init=0.0, ortho_init=True, device="cpu"):
        self.obs_dim, self.act_dim, self.depth, self.separate = int(obs_dim), int(act_dim), int(depth), bool(separate)
        self.log_std_init, self.ortho_init = float(log_std_init), bool(ortho_init)
        super().__init__(*param_layout(obs_dim, act_dim, depth, separate), seed, device)

    def _init_linear(self, name, lin):
        if self.ortho_init:
            gain = {"trunk": math.sqrt(2.0), "action_net": 0.01, "value_net": 1.0}[group_of(name)]
            self.torch.nn.init.orthogonal_(lin.weight, gain=gain)
            lin.bias.data.fill_(0.0)

    def _init_rest(self, flat):
        off, _ = self.layout["log_std"]
        flat[off:off + self.act_dim] = self.log_std_init

    def group(self, flat, which):
        """The entries of a parameter-shaped vector that belong to "trunk" (every hidden layer), "action_net", "value_net" or "log_std", in the layout's order."""
        return self.torch.cat([flat[off:off + int(np.prod(shape))] for name, (off, shape) in self.layout.items() if group_of(name) == which])


class PpoLearner(Learner):
    """SB3's PPO update on the device for the shapes the kernels cover (`build_ppo_desc` refuses the rest).  `learning_rate`, `clip_range` and `clip_range_vf`
    (None: the value function is not clipped) are plain attributes, passed with every step: a caller may schedule them.  All tensor arguments and results live
    on the learner's device; `step`, `train`, `policy` and `value` are asynchronous, ordered on torch's current stream; `diagnostics` and `export` synchronise."""

    _prefix = "hrg_ppo"
    n_members = 1   # (PpoPopulation: more)

    def __init__(self, obs_dim, act_dim, net_arch=None, learning_rate=3e-4, batch_size=64, n_epochs=10, clip_range=0.2, clip_range_vf=None, normalize_advantage=True,
                 ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, use_sde=False, target_kl=None, policy="MlpPolicy", log_std_init=0.0, ortho_init=True, rollout_size=0,
                 seed=0, device=0, **policy_kwargs):
        unknown = sorted(set(policy_kwargs) - set(IGNORED_POLICY_KWARGS))
        if unknown:
            raise NotImplementedError(f"policy_kwargs {unknown}: the device learner takes net_arch, log_std_init, ortho_init (and ignores {list(IGNORED_POLICY_KWARGS)} while use_sde is false)")
        if int(n_epochs) < 1:
            raise ValueError(f"n_epochs = {n_epochs} must be positive")
        desc = build_ppo_desc(obs_dim, act_dim, net_arch=net_arch, batch_size=batch_size, rollout_size=rollout_size, normalize_advantage=normalize_advantage,
                              ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm, use_sde=use_sde, target_kl=target_kl, policy=policy, seed=seed)
        self._kwargs = dict(net_arch=net_arch, batch_size=batch_size, normalize_advantage=normalize_advantage, ent_coef=ent_coef, vf_coef=vf_coef,
                            max_grad_norm=max_grad_norm, rollout_size=rollout_size, log_std_init=log_std_init, ortho_init=ortho_init)   # (a population's member())
        self._open_handle(desc, device)
        self.obs_dim, self.act_dim, self.depth, self.separate = int(obs_dim), int(act_dim), int(desc.depth), bool(desc.separate)
        self.batch_size, self.n_epochs = int(batch_size), int(n_epochs)
        self.learning_rate, self.clip_range = float(learning_rate), float(clip_range)
        self.clip_range_vf = None if clip_range_vf is None else float(clip_range_vf)
        self.p = self._make_params(seed, log_std_init, ortho_init)
        if self._sizes()[0] != self.p.n_params:
            raise RuntimeError(f"{type(self).__name__}: the library lays out {self._sizes()[0]} parameters, ppo.param_layout {self.p.n_params}: rebuild")
        self._keep = None

    def _open_handle(self, desc, device):
        self._open(desc, device)

    def _make_params(self, seed, log_std_init, ortho_init):
        return PpoParams(self.obs_dim, self.act_dim, self.depth, self.separate, seed=seed, log_std_init=log_std_init, ortho_init=ortho_init, device=self.device)

    def _hyper(self):
        return dict(learning_rate=self.learning_rate, clip_range=self.clip_range, clip_range_vf=self.clip_range_vf, n_epochs=self.n_epochs)

    @staticmethod
    def _checkpoint_kwargs(d, hyper):
        """The constructor's arguments, the seed apart, from a checkpoint's descriptor fields `d` and scheduled attributes `hyper`.  log_std_init and ortho_init
        shape the initial parameters only, which the checkpoint's replace."""
        layers = [int(d["hidden"])] * int(d["depth"])
        vf = float(hyper["clip_range_vf"])
        return dict(obs_dim=int(d["obs_dim"]), act_dim=int(d["act_dim"]), net_arch=[dict(pi=layers, vf=list(layers))] if int(d["separate"]) else layers,
                    learning_rate=float(hyper["learning_rate"]), batch_size=int(d["batch_size"]), n_epochs=int(hyper["n_epochs"]), clip_range=float(hyper["clip_range"]),
                    clip_range_vf=None if math.isnan(vf) else vf, normalize_advantage=bool(int(d["normalize_advantage"])), ent_coef=float(d["ent_coef"]),
                    vf_coef=float(d["vf_coef"]), max_grad_norm=float(d["max_grad_norm"]), rollout_size=int(d["rollout_size"]))

    @classmethod
    def _from_checkpoint(cls, d, hyper, device):
        """The learner of a checkpoint's descriptor fields `d` and scheduled attributes `hyper` (Learner.load)."""
        return cls(seed=int(d["seed"]), device=device, **cls._checkpoint_kwargs(d, hyper))

    def step(self, batch):
        """One minibatch step on `batch`, a RolloutBufferSamples of `batch_size` rows (observations [B, obs_dim], actions [B, act_dim], old_values,
        old_log_prob, advantages, returns [B]).  A population takes its members' minibatches one behind the other, [P * B] rows."""
        B, K, A, p = self.n_members * self.batch_size, self.obs_dim, self.act_dim, self.p
        lr, clip, clip_vf = self._step_scalars()
        if clip_vf is not None and not clip_vf > 0.0:
            raise ValueError(f"clip_range_vf = {clip_vf} must be positive (None: no clipping)")
        args = (self._tensor(batch.observations, (B, K), "observations"), self._tensor(batch.actions, (B, A), "actions"), self._tensor(batch.old_values, (B,), "old_values"),
                self._tensor(batch.old_log_prob, (B,), "old_log_prob"), self._tensor(batch.advantages, (B,), "advantages"), self._tensor(batch.returns, (B,), "returns"))
        with self.torch.cuda.device(self.device):
            self._check(self.lib, self.lib.hrg_ppo_step(self.h, *args, _ptr(p.params), _ptr(p.adam_m), _ptr(p.adam_v), float(lr), float(clip),
                                                         -1.0 if clip_vf is None else float(clip_vf), self._stream()))
        self._keep = batch

    def _step_scalars(self):
        """learning_rate, clip_range, clip_range_vf as `step` passes them."""
        return self.learning_rate, self.clip_range, self.clip_range_vf

    def train(self, rollout):
        """PPO.train: `n_epochs` x (rollout.get(batch_size) -> step), with no copy to the host and no synchronisation.  batch_size must divide the buffer's
        n_envs * n_steps: the learner takes no short last minibatch."""
        self._check_buffer(rollout.obs_dim, rollout.act_dim)
        N =int(rollout.n) * int(rollout.n_steps)
        if N % self.batch_size:
            raise NotImplementedError(f"train: batch_size = {self.batch_size} does not divide n_envs * n_steps = {N}: the learner takes no short last minibatch")
        for _ in range(self.n_epochs):
            for batch in rollout.get(self.batch_size):
                self.step(batch)

    def _forward(self, obs, eps, deterministic, with_actions):
        """(actions, values, log_probs) on `obs` [n, obs_dim]; a population: [P m, obs_dim], member p's networks on the rows of group p."""
        t = self.torch
        n, o, e = self._rows(obs, eps)
        if n % self.n_members:
            raise ValueError(f"forward: {n} rows are not {self.n_members} groups of the same size")
        values =t.empty(n, dtype=t.float32, device=self.device)
        actions = t.empty(n, self.act_dim, dtype=t.float32, device=self.device) if with_actions else None
        log_probs = t.empty(n, dtype=t.float32, device=self.device) if with_actions else None
        with t.cuda.device(self.device):   # (hrg_ppo_forward is this entry for one member)
            self._check(self.lib, self.lib.hrg_ppo_population_forward(self.h, _ptr(self.p.params), o, n // self.n_members, e, int(bool(deterministic)), _ptr(actions),
                                                                       _ptr(values), _ptr(log_probs), self._stream()))
        return actions, values, log_probs

    def policy(self, obs, deterministic=False, eps=None):
        """ActorCriticPolicy.forward on `obs` float32 [n, obs_dim]: (actions float32 [n, act_dim], values [n], log_probs [n]); actions = mu + exp(log_std) eps,
        not clipped (collect_rollout clips what the env gets), or mu with `deterministic`.  This is the `policy` HipVecEnv.collect_rollout takes.  `eps` float32
        [n, act_dim] replaces the draws (tests)."""
        return self._forward(obs, eps, deterministic, True)

    def value(self, obs):
        """ActorCriticPolicy.predict_values on `obs` float32 [n, obs_dim]: float32 [n].  This is the `value_fn` HipVecEnv.collect_rollout takes."""
        return self._forward(obs, None, True, False)[1]

    def export(self, **which):
        """The last step's intermediates on the host (synchronous; tests): values, log_prob, ratio [B]; grad [n_params] in the parameters' layout, before
        clipping (`self.p.group(grad, "trunk")`, ...); diag: dict of DIAG_KEYS.  (`which`: PpoPopulation's `member`.)"""
        B = self.batch_size
        values, log_prob, ratio = np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
        grad, diag = np.zeros(self.p.n_params, np.float32), np.zeros(NDIAG, np.float32)
        self._export(values, log_prob, ratio, grad, diag, **which)
        return dict(values=values, log_prob=log_prob, ratio=ratio, grad=grad, diag=dict(zip(DIAG_KEYS, (float(x) for x in diag))))

    def diagnostics(self, **which):
        """What SB3 logs under train/ after a call of train(), from the last minibatch: policy_gradient_loss, value_loss, entropy_loss, loss, approx_kl,
        clip_fraction, std, plus grad_norm (before clipping), clip_range, clip_range_vf where set, learning_rate and n_updates.  Synchronous."""
        diag = np.zeros(NDIAG, np.float32)
        self._export(None, None, None, None, diag, **which)
        out = dict(zip(DIAG_KEYS, (float(x) for x in diag)))
        out.update(clip_range=self._scalar("clip_range", **which), learning_rate=self._scalar("learning_rate", **which), n_updates=self.n_updates)
        if self._scalar("clip_range_vf", **which) is not None:
            out["clip_range_vf"] = self._scalar("clip_range_vf", **which)
        return out


class PpoPopulationParams(PopulationParams):
    """The tensors of a population, on any torch device: `params`, `adam_m`, `adam_v` float32 [P, n_params].  Row p is initialised exactly as
    PpoParams(seed=seeds[p], ...); `member(p)` is the rows of member p as views."""

    def __init__(self, obs_dim, act_dim, depth, separate, seeds, log_std_init=0.0, ortho_init=True, device="cpu"):
        super().__init__([PpoParams(obs_dim, act_dim, depth, separate, seed=int(s), log_std_init=log_std_init, ortho_init=ortho_init) for s in seeds], device)


class PpoPopulation(Population, PpoLearner):
    """`n_members` PPO learners of the same shapes (PpoLearner's keywords) that take their minibatch step in the same four launches (csrc/hrgym_ppo.h;
    DESIGN.md D29, D30): the seeds of one cell of a study, or the cells of a sweep, side by side on one GPU.  The batch of n = P m envs is P groups of m
    consecutive envs; member p acts in, and learns from, group p only.  The counters are shared: members step in lockstep.  `learning_rate`, `clip_range`,
    `clip_range_vf` (None: not clipped), `ent_coef`, `vf_coef` and `max_grad_norm` take a scalar (every member) or a sequence of one value per member; the first
    three may be assigned between steps, a scalar or a sequence.  What shapes a launch, the lockstep or the host's loop is shared (`_shared`).  Member p is, bit
    for bit, PpoLearner(seed=seeds[p], **member_hyper(p)) on the same rows.  `rollout_size`: m * n_steps, a member's share of the buffer.  export(member),
    diagnostics (a list of P dicts), member(p), member_hyper(p), save and load (member_<p>.npz and, where the members differ, population.npz):
    _learner.Population.

        env.attach_rollout(n_steps=64, gamma=0.99, gae_lambda=0.9)
        pop = env.attach_ppo_population(5, batch_size=64)            # seeds: the env's seed + p
        env.collect_rollout(pop.policy, pop.value)
        pop.train(env.rollout)
        pop.diagnostics()                                            # a list of 5 dicts
    """
    _lone = PpoLearner
    _fields = ("learning_rate", "clip_range", "clip_range_vf", "ent_coef", "vf_coef", "max_grad_norm")
    _scheduled = ("learning_rate", "clip_range", "clip_range_vf")
    _manifest_fields = _fields
    learning_rate, clip_range, clip_range_vf = (scheduled_attribute(name) for name in _scheduled)
    _defaults = dict(learning_rate=3e-4, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)   # PpoLearner's
    _shared = dict(net_arch="the depth and the trunks shape every launch", batch_size="the minibatch shapes every launch", n_epochs="the epochs are the host's loop over all members",
                   normalize_advantage="it decides whether the advantage kernel is launched", rollout_size="the members' shares of the buffer are equal",
                   log_std_init="it shapes the initial parameters, not the step", ortho_init="it shapes the initial parameters, not the step",
                   use_sde="not covered", target_kl="not covered", policy="one policy class per handle")

    def __init__(self, obs_dim, act_dim, n_members, seeds, device=0, **kwargs):
        self.n_members, self._table = check_seeds(n_members, seeds)
        self.seeds = [int(s) for s in self._table]
        if "seed" in kwargs:
            raise TypeError("PpoPopulation: the members' seeds are `seeds` (one per member), not `seed`")
        refuse_shared_sequences(self._shared, kwargs)
        values = {name: kwargs.pop(name, self._defaults[name]) for name in self._fields}
        self._set_values(**values)   # (every member's values are checked before anything is allocated)
        first = self.member_hyper(0)
        super().__init__(obs_dim, act_dim, seed=self.seeds[0], device=device, **first, **kwargs)   # (the entry reads the table, not the descriptor's seed)
        self._set_values(**values)   # (the lone learner's constructor assigned member 0's scheduled attributes to all)
        self._sync_table()

    @staticmethod
    def _convert(name, value):
        """One member's value of a table field as the constructor takes it; ValueError for what no learner takes."""
        if name == "clip_range_vf" and value is None:
            return None
        value = float(value)
        positive = name in ("clip_range", "clip_range_vf", "max_grad_norm")
        if not math.isfinite(value) or value < 0.0 or (positive and value == 0.0):
            raise ValueError(f"{name} = {value} must be finite and {'positive' if positive else 'not negative'}" + (" (None: no clipping)" if name == "clip_range_vf" else ""))
        return value

    def _step_scalars(self):
        """Member 0's, kept as a tuple: `step` runs once per minibatch, and the library reads its table once that is the caller's."""
        return self._member0

    def _member_desc(self, p):
        """Member p's descriptor: the lone learner's of its seed and its values."""
        desc, v = type(self.desc).from_buffer_copy(self.desc), self.member_hyper(p)
        desc.seed, desc.ent_coef, desc.vf_coef, desc.max_grad_norm = self.seeds[p], v["ent_coef"], v["vf_coef"], v["max_grad_norm"]
        return desc

    def _row(self, p):
        return self.table_row(self.member_hyper(p))

    @staticmethod
    def table_row(v):
        """hrg_ppo_hyper of one member's values `v` (member_hyper's dict): clip_range_vf None is the negative sentinel."""
        row = PpoHyper()
        row.learning_rate, row.clip_range, row.clip_range_vf = v["learning_rate"], v["clip_range"], -1.0 if v["clip_range_vf"] is None else v["clip_range_vf"]
        row.ent_coef, row.vf_coef, row.max_grad_norm = v["ent_coef"], v["vf_coef"], v["max_grad_norm"]
        return row

    def _open_handle(self, desc, device):
        self._open(desc, device, self.n_members, self._table.ctypes.data_as(ctypes.c_void_p), create="_population_create")

    def _make_params(self, seed, log_std_init, ortho_init):
        return PpoPopulationParams(self.obs_dim, self.act_dim, self.depth, self.separate, self.seeds, log_std_init=log_std_init, ortho_init=ortho_init, device=self.device)

    def train(self, rollout):
        """PPO.train of every member: `n_epochs` x (rollout.get_groups(n_members, batch_size, seeds) -> step), with no copy to the host and no
        synchronisation.  `rollout`: a rollout.RolloutBuffer over n_members groups of envs; batch_size must divide a group's m * n_steps rows."""
        self._check_buffer(rollout.obs_dim, rollout.act_dim)
        for _ in range(self.n_epochs):
            for batch in rollout.get_groups(self.n_members, self.batch_size, self.seeds):
                self.step(batch)
