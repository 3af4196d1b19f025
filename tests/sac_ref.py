"""One gradient step of SB3 1.5.0's SAC.train (use_sde=False), restated with torch autograd on the CPU ([UPSTREAM]: written out from knowledge of that release;
stable-baselines3 is not a dependency).  Parameterised by dtype, with explicit batch, noise, parameters and Adam state: `ref64` is a float64 run and `ref32` a
float32 run of the same code; their difference is the float32 noise floor the device results are held against (tests/test_sac_gpu.py).  Nothing here reads the
code under test: parameters are a plain dict under SB3's names.

    state = RefState(params, dtype)                    # params: dict name -> array-like, SB3's names (actor.*, critic.*, critic_target.*, log_ent_coef)
    out = state.step(batch, eps_pi, eps_next, cfg)     # batch: dict observations, actions, next_observations, dones, rewards;  cfg: Cfg(...)
    out["y"], out["logp"], out["logp_next"], out["q"] (dict of the six Q columns), out["grad"] (dict name -> gradient), out["losses"]
"""
import math
from collections import OrderedDict, namedtuple

import torch

Cfg = namedtuple("Cfg", ["depth", "lr", "gamma", "tau", "auto_ent_coef", "ent_coef", "target_entropy", "target_update_interval"])
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0   # stable_baselines3/sac/policies.py
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def mlp(p, prefix, x, depth):
    """create_mlp's Sequential: Linear, ReLU, ... at indices 0, 2, ..; returns the last hidden activation."""
    for l in range(depth):
        x = torch.relu(torch.nn.functional.linear(x, p[f"{prefix}.{2 * l}.weight"], p[f"{prefix}.{2 * l}.bias"]))
    return x


def actor_heads(p, obs, depth):
    """mu and the clamped log_std of the actor (Actor.get_action_dist_params), and the log_std head before the clamp."""
    h = mlp(p, "actor.latent_pi", obs, depth)
    mu = torch.nn.functional.linear(h, p["actor.mu.weight"], p["actor.mu.bias"])
    raw = torch.nn.functional.linear(h, p["actor.log_std.weight"], p["actor.log_std.bias"])
    return mu, torch.clamp(raw, LOG_STD_MIN, LOG_STD_MAX), raw


def squashed_logp(mu, log_std, eps):
    """a = tanh(mu + exp(log_std) eps) and its log probability: sum_j [-0.5 eps_j^2 - log_std_j - 0.5 log(2 pi)] - sum_j log(1 - a_j^2 + 1e-6)
    (SquashedDiagGaussianDistribution.log_prob_from_params with the sample written as mu + std eps)."""
    a = torch.tanh(mu + torch.exp(log_std) * eps)
    logp = (-0.5 * eps * eps - log_std - 0.5 * math.log(2.0 * math.pi)).sum(-1) - torch.log(1.0 - a * a + 1e-6).sum(-1)
    return a, logp


def actor(p, obs, eps, depth):
    mu, log_std, _ = actor_heads(p, obs, depth)
    return squashed_logp(mu, log_std, eps)


def q_value(p, prefix, obs, act, depth):
    """ContinuousCritic's q network `prefix` on concat(obs, act): [B]."""
    h = mlp(p, prefix, torch.cat([obs, act], dim=-1), depth)
    return torch.nn.functional.linear(h, p[f"{prefix}.{2 * depth}.weight"], p[f"{prefix}.{2 * depth}.bias"]).squeeze(-1)


def adam_update(p, g, m, v, t, lr):
    """torch.optim.Adam's step t (counted from 1) on one tensor, in place: betas (0.9, 0.999), eps 1e-8, no weight decay.  Returns the update's size
    m_hat / (sqrt(v_hat) + eps)."""
    m.mul_(BETA1).add_(g, alpha=1.0 - BETA1)
    v.mul_(BETA2).addcmul_(g, g, value=1.0 - BETA2)
    upd = (m / (1.0 - BETA1 ** t)) / ((v / (1.0 - BETA2 ** t)).sqrt() + ADAM_EPS)
    p.sub_(lr * upd)
    return upd


class RefState:
    """Parameters, targets, Adam moments and the step count of one learner in `dtype`."""

    def __init__(self, params, dtype, device="cpu"):
        self.dtype, self.device = dtype, torch.device(device)   # (a device other than the CPU: tools/bench_sac.py times this code as the eager baseline)
        self.p = OrderedDict((k, torch.as_tensor(v).detach().to(self.device, dtype).clone()) for k, v in params.items())
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items() if not k.startswith("critic_target.")}
        self.v = {k: torch.zeros_like(v) for k, v in self.m.items()}
        self.steps = 0

    def names(self, prefix):
        return [k for k in self.p if k.startswith(prefix)]

    def step(self, batch, eps_pi, eps_next, cfg, outputs=True):
        """One gradient step; `batch` is a dict or a ReplayBufferSamples-like object.  `outputs=False` returns nothing (and copies nothing)."""
        p, dt, depth = self.p, self.dtype, cfg.depth
        if not isinstance(batch, dict):
            batch = batch._asdict()
        cast = lambda x: torch.as_tensor(x).detach().to(self.device, dt)   # noqa: E731
        obs, act, nobs = cast(batch["observations"]), cast(batch["actions"]), cast(batch["next_observations"])
        d, r = cast(batch["dones"]).reshape(-1), cast(batch["rewards"]).reshape(-1)
        eps_pi, eps_next = cast(eps_pi), cast(eps_next)
        t = self.steps + 1
        grad = {}
        for k in self.m:
            p[k].requires_grad_(True)
        # 1: the actor on the batch
        a_pi, logp = actor(p, obs, eps_pi, depth)
        # 2: the entropy coefficient, taken before its update
        if cfg.auto_ent_coef:
            alpha = torch.exp(p["log_ent_coef"].detach())[0]
            ent_loss = -(p["log_ent_coef"] * (logp.detach() + cfg.target_entropy)).mean()
            grad["log_ent_coef"], = torch.autograd.grad(ent_loss, [p["log_ent_coef"]])
        else:
            alpha, ent_loss = torch.tensor(cfg.ent_coef, dtype=dt, device=self.device), torch.zeros((), dtype=dt, device=self.device)
        # 3: the critics
        with torch.no_grad():
            a_next, logp_next = actor(p, nobs, eps_next, depth)
            q1t, q2t = q_value(p, "critic_target.qf0", nobs, a_next, depth), q_value(p, "critic_target.qf1", nobs, a_next, depth)
            y = r + (1.0 - d) * cfg.gamma * (torch.min(q1t, q2t) - alpha * logp_next)
        q1, q2 = q_value(p, "critic.qf0", obs, act, depth), q_value(p, "critic.qf1", obs, act, depth)
        critic_loss = 0.5 * (((q1 - y) ** 2).mean() + ((q2 - y) ** 2).mean())
        cn = self.names("critic.")
        for k, g in zip(cn, torch.autograd.grad(critic_loss, [p[k] for k in cn])):
            grad[k] = g
        upd = {}
        with torch.no_grad():
            for k in cn:
                upd[k] = adam_update(p[k], grad[k], self.m[k], self.v[k], t, cfg.lr)
        # 4: the actor, through the updated critics
        q1p, q2p = q_value(p, "critic.qf0", obs, a_pi, depth), q_value(p, "critic.qf1", obs, a_pi, depth)
        actor_loss = (alpha * logp - torch.min(q1p, q2p)).mean()
        an = self.names("actor.")
        for k, g in zip(an, torch.autograd.grad(actor_loss, [p[k] for k in an])):
            grad[k] = g
        with torch.no_grad():
            for k in an:
                upd[k] = adam_update(p[k], grad[k], self.m[k], self.v[k], t, cfg.lr)
            if cfg.auto_ent_coef:
                upd["log_ent_coef"] = adam_update(p["log_ent_coef"], grad["log_ent_coef"], self.m["log_ent_coef"], self.v["log_ent_coef"], t, cfg.lr)
            # 5: the targets
            if self.steps % cfg.target_update_interval == 0:
                for k in cn:
                    tk = "critic_target." + k[len("critic."):]
                    p[tk].mul_(1.0 - cfg.tau).add_(p[k], alpha=cfg.tau)
        for k in self.m:
            p[k].requires_grad_(False)
        self.steps += 1
        if not outputs:
            return None
        det = lambda x: x.detach().clone()   # noqa: E731
        return dict(y=det(y), logp=det(logp), logp_next=det(logp_next), a_pi=det(a_pi),
                    q=OrderedDict(q1=det(q1), q2=det(q2), q1_target=det(q1t), q2_target=det(q2t), q1_pi=det(q1p), q2_pi=det(q2p)),
                    grad={k: det(g) for k, g in grad.items()}, update=upd,
                    losses=dict(actor_loss=float(actor_loss.detach()), critic_loss=float(critic_loss.detach()), ent_coef_loss=float(ent_loss.detach()), ent_coef=float(alpha)))

    def act(self, obs, eps=None):
        """tanh(mu + std eps), or tanh(mu) without eps."""
        with torch.no_grad():
            mu, log_std, _ = actor_heads(self.p, torch.as_tensor(obs).to(self.device, self.dtype), self.depth_hint)
            return torch.tanh(mu if eps is None else mu + torch.exp(log_std) * torch.as_tensor(eps).to(self.device, self.dtype))

    @property
    def depth_hint(self):
        return sum(1 for k in self.p if k.startswith("actor.latent_pi.") and k.endswith(".weight"))


# ---- the cases of the tests: parameters and batches built so that every branch of the step is met
def make_params(obs_dim, act_dim, depth, seed, target_noise=0.05):
    """Parameters under SB3's names with torch.nn.Linear's bounds (uniform in +-1/sqrt(fan_in)), float64 tensors holding float32 values; the targets are the
    critics plus a perturbation, so that a target that was read in place of a critic shows."""
    g = torch.Generator().manual_seed(int(seed))
    p = OrderedDict()

    def linear(name, out, inp):
        bound = 1.0 / math.sqrt(inp)
        p[name + ".weight"] = (torch.rand(out, inp, generator=g, dtype=torch.float64) * 2.0 - 1.0) * bound
        p[name + ".bias"] = (torch.rand(out, generator=g, dtype=torch.float64) * 2.0 - 1.0) * bound

    for l in range(depth):
        linear(f"actor.latent_pi.{2 * l}", 64, 64 if l else obs_dim)
    linear("actor.mu", act_dim, 64)
    linear("actor.log_std", act_dim, 64)
    for q in range(2):
        for l in range(depth):
            linear(f"critic.qf{q}.{2 * l}", 64, 64 if l else obs_dim + act_dim)
        linear(f"critic.qf{q}.{2 * depth}", 1, 64)
    for k in [k for k in p if k.startswith("critic.")]:
        p["critic_target." + k[len("critic."):]] = p[k] + target_noise * (torch.rand(p[k].shape, generator=g, dtype=torch.float64) * 2.0 - 1.0) * p[k].abs().max()
    p["log_ent_coef"] = torch.tensor([math.log(0.2)], dtype=torch.float64)
    return OrderedDict((k, v.float().double()) for k, v in p.items())


def make_case(obs_dim, act_dim, depth, batch, seed):
    """(params, batch, eps_pi, eps_next) that meet every branch: dead ReLU units in the first layer of the actor and of both critics (bias -50), min(Q1, Q2) picking either, a log_std head
    whose entries clamp at +2, at -20 and not at all (with act_dim >= 3: column 0 clamps at +2 and column 1 at -20 in every row), both values of `dones`.
    The noise is bounded by 0.45: with std = exp(2) the squashed action then stays away from +-1, where log(1 - a^2 + 1e-6) loses every digit in float32."""
    g = torch.Generator().manual_seed(int(seed) + 1000)
    p = make_params(obs_dim, act_dim, depth, seed)
    p["actor.latent_pi.0.bias"][[3, 17]] = -50.0
    p["critic.qf0.0.bias"][[5]] = -50.0
    p["critic.qf1.0.bias"][[9, 40]] = -50.0
    p["critic_target.qf0.0.bias"][[5]] = -50.0
    p["critic_target.qf1.0.bias"][[9, 40]] = -50.0
    normal = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)   # noqa: E731
    obs = normal(batch, obs_dim).float().double()
    # the log_std head.  Three actions or more: the bias puts column 0 above +2 and column 1 below -20 in every row, the other columns stay where the initial
    # weights put them, unclamped.  Fewer: the only way to meet all three branches is across the rows, so row j of the layer is scaled and shifted until its
    # quartiles over the batch sit near -22 and +4 and its median at -9 (a head with weights near 100, which magnifies float32 rounding in log_std and makes
    # the float32 floor of such a case correspondingly higher).
    if act_dim >= 3:
        p["actor.log_std.bias"][0], p["actor.log_std.bias"][1] = 10.0, -30.0
    else:
        z = mlp(p, "actor.latent_pi", obs, depth) @ p["actor.log_std.weight"].T
        for j in range(act_dim):
            q25, med, q75 = (torch.quantile(z[:, j], x) for x in (0.25, 0.5, 0.75))
            scale = 13.0 / max(float(min(q75 - med, med - q25)), 1e-9)
            p["actor.log_std.weight"][j] *= scale
            p["actor.log_std.bias"][j] = -9.0 - scale * med
    p = OrderedDict((k, v.float().double()) for k, v in p.items())
    b = dict(observations=obs, actions=torch.rand(batch, act_dim, generator=g, dtype=torch.float64) * 2.0 - 1.0,
             next_observations=normal(batch, obs_dim), dones=(torch.rand(batch, 1, generator=g) < 0.3).double(), rewards=normal(batch, 1))
    eps_pi, eps_next = (0.3 * normal(batch, act_dim)).clamp(-0.45, 0.45), (0.3 * normal(batch, act_dim)).clamp(-0.45, 0.45)
    f32 = lambda x: x.float().double()   # noqa: E731
    b, eps_pi, eps_next = {k: f32(v) for k, v in b.items()}, f32(eps_pi), f32(eps_next)
    # the second critic's output bias, moved so that min(Q1, Q2) picks each of them in half of the rows: the targets on (next_obs, a'), the critics on (obs, a_pi)
    out = f"{2 * depth}.bias"
    for prefix, obs, eps in (("critic_target", b["next_observations"], eps_next), ("critic", b["observations"], eps_pi)):
        a, _ = actor(p, obs, eps, depth)
        p[f"{prefix}.qf1.{out}"] += (q_value(p, f"{prefix}.qf0", obs, a, depth) - q_value(p, f"{prefix}.qf1", obs, a, depth)).median()
        p[f"{prefix}.qf1.{out}"] = f32(p[f"{prefix}.qf1.{out}"])
    return p, b, eps_pi, eps_next


def assert_branches(params, batch, eps_pi, eps_next, out64, depth):
    """Every branch the case is built for occurs in the float64 run."""
    p = {k: torch.as_tensor(v).double() for k, v in params.items()}
    d = batch["dones"].reshape(-1)
    assert (d == 0).any() and (d == 1).any(), "both values of dones"
    q = out64["q"]
    for a, b in (("q1_target", "q2_target"), ("q1_pi", "q2_pi")):
        assert (q[a] < q[b]).any() and (q[a] > q[b]).any(), f"min picks both of {a}, {b}"
    obs, act = batch["observations"], batch["actions"]
    for prefix, x in (("actor.latent_pi", obs), ("critic.qf0", torch.cat([obs, act], -1)), ("critic.qf1", torch.cat([obs, act], -1))):
        h = mlp(p, prefix, x, 1)
        assert ((h == 0).all(dim=0)).any(), f"{prefix}: a unit that is dead over the whole batch"
    _, _, raw = actor_heads(p, obs, depth)
    assert (raw > LOG_STD_MAX).any() and (raw < LOG_STD_MIN).any() and ((raw > LOG_STD_MIN) & (raw < LOG_STD_MAX)).any(), "log_std clamps at both ends and not at all"
