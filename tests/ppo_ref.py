"""One minibatch step of SB3 1.5.0's PPO.train with ActorCriticPolicy.evaluate_actions (MlpPolicy, use_sde=False, Box actions), restated from torch's own parts
([UPSTREAM]: written out from knowledge of that release; stable-baselines3 is not a dependency): autograd, torch.distributions.Normal,
torch.nn.utils.clip_grad_norm_ and torch.optim.Adam(eps=1e-5).  Nothing in it is hand-derived.  Parameterised by dtype, with explicit batch and parameters:
`ref64` is a float64 run and `ref32` a float32 run of the same code; their difference is the float32 noise floor the device results are held against
(tests/test_ppo_gpu.py).  Nothing here reads the code under test: parameters are a plain dict under SB3's names, in the order of the device's parameter vector
(tests/test_ppo.py holds `layout` against ppo.param_layout).

    state = RefState(params, dtype)          # params: dict name -> array-like (make_params)
    out = state.step(batch, cfg)             # batch: dict or namedtuple of observations, actions, old_values, old_log_prob, advantages, returns;  cfg: Cfg(...)
    out["values"], out["log_prob"], out["ratio"], out["grad"] (dict name -> gradient before clipping), out["grad_norm"], out["losses"]
"""
import math
from collections import OrderedDict, namedtuple

import torch

Cfg = namedtuple("Cfg", ["depth", "separate", "lr", "clip_range", "clip_range_vf", "normalize_advantage", "ent_coef", "vf_coef", "max_grad_norm"])
ADAM_EPS = 1e-5   # PPO's policy optimiser: optimizer_kwargs eps = 1e-5
FIELDS = ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns")


def layout(obs_dim, act_dim, depth, separate):
    """name -> shape, in the order of the device's parameter vector."""
    out = OrderedDict()
    for net in (("policy_net", "value_net") if separate else ("shared_net",)):
        for l in range(depth):
            out[f"mlp_extractor.{net}.{2 * l}.weight"] = (64, 64 if l else obs_dim)
            out[f"mlp_extractor.{net}.{2 * l}.bias"] = (64,)
    out["action_net.weight"], out["value_net.weight"], out["action_net.bias"], out["value_net.bias"], out["log_std"] = (act_dim, 64), (1, 64), (act_dim,), (1,), (act_dim,)
    return out


def latent(p, net, x, depth):
    """MlpExtractor's Sequential: Linear, Tanh, ... at indices 0, 2, .."""
    for l in range(depth):
        x = torch.tanh(torch.nn.functional.linear(x, p[f"mlp_extractor.{net}.{2 * l}.weight"], p[f"mlp_extractor.{net}.{2 * l}.bias"]))
    return x


def heads(p, obs, depth, separate):
    """(mu [B, A], values [B]) of ActorCriticPolicy.forward."""
    lp = latent(p, "policy_net" if separate else "shared_net", obs, depth)
    lv = latent(p, "value_net", obs, depth) if separate else lp
    mu = torch.nn.functional.linear(lp, p["action_net.weight"], p["action_net.bias"])
    return mu, torch.nn.functional.linear(lv, p["value_net.weight"], p["value_net.bias"]).squeeze(-1)


def distribution(p, mu):
    """DiagGaussianDistribution.proba_distribution: Normal(mu, ones_like(mu) * exp(log_std))."""
    return torch.distributions.Normal(mu, torch.ones_like(mu) * p["log_std"].exp())


def evaluate_actions(p, obs, actions, depth, separate):
    """ActorCriticPolicy.evaluate_actions: values, log_prob, entropy (sum_independent_dims over the action's components)."""
    mu, values = heads(p, obs, depth, separate)
    dist = distribution(p, mu)
    return values, dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)


def log_prob_closed_form(mu, log_std, actions):
    """sum_j [-(a_j - mu_j)^2 / (2 exp(2 log_std_j)) - log_std_j - 0.5 log 2 pi], written by hand: the anchor of tests/test_ppo.py."""
    return (-(actions - mu) ** 2 / (2.0 * torch.exp(2.0 * log_std)) - log_std - 0.5 * math.log(2.0 * math.pi)).sum(-1)


def entropy_closed_form(log_std):
    return (0.5 + 0.5 * math.log(2.0 * math.pi) + log_std).sum(-1)


def losses(p, batch, cfg):
    """The losses of one minibatch as PPO.train computes them; returns (loss, dict of the tensors behind it)."""
    values, log_prob, entropy = evaluate_actions(p, batch["observations"], batch["actions"], cfg.depth, cfg.separate)
    adv = batch["advantages"]
    if cfg.normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(log_prob - batch["old_log_prob"])
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1.0 - cfg.clip_range, 1.0 + cfg.clip_range)).mean()
    clip_fraction = torch.mean((torch.abs(ratio - 1.0) > cfg.clip_range).to(ratio.dtype))
    if cfg.clip_range_vf is None:
        values_pred = values
    else:
        values_pred = batch["old_values"] + torch.clamp(values - batch["old_values"], -cfg.clip_range_vf, cfg.clip_range_vf)
    value_loss = torch.nn.functional.mse_loss(batch["returns"], values_pred)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + cfg.ent_coef * entropy_loss + cfg.vf_coef * value_loss
    with torch.no_grad():
        log_ratio = log_prob - batch["old_log_prob"]
        approx_kl = torch.mean((torch.exp(log_ratio) - 1.0) - log_ratio)
    return loss, dict(values=values, log_prob=log_prob, ratio=ratio, policy_gradient_loss=policy_loss, value_loss=value_loss, entropy_loss=entropy_loss, loss=loss,
                      approx_kl=approx_kl, clip_fraction=clip_fraction, std=p["log_std"].exp().mean())


def as_batch(batch, dtype, device="cpu"):
    if not isinstance(batch, dict):
        batch = batch._asdict()
    return {k: torch.as_tensor(batch[k]).detach().to(device, dtype) for k in FIELDS}


class RefState:
    """Parameters, torch.optim.Adam and the step count of one learner in `dtype`."""

    def __init__(self, params, dtype, device="cpu"):
        self.dtype, self.device = dtype, torch.device(device)   # (a device other than the CPU: tools/bench_ppo.py times this code as the eager baseline)
        self.p = OrderedDict((k, torch.nn.Parameter(torch.as_tensor(v).detach().to(self.device, dtype).clone())) for k, v in params.items())
        self.opt = torch.optim.Adam(list(self.p.values()), lr=1.0, eps=ADAM_EPS)
        self.steps = 0

    def step(self, batch, cfg, outputs=True):
        """One minibatch step.  `outputs=False` returns nothing (and copies nothing)."""
        b = as_batch(batch, self.dtype, self.device)
        for g in self.opt.param_groups:
            g["lr"] = cfg.lr
        loss, t = losses(self.p, b, cfg)
        self.opt.zero_grad()
        loss.backward()
        grad = {k: v.grad.detach().clone() for k, v in self.p.items()} if outputs else None
        norm = torch.nn.utils.clip_grad_norm_(list(self.p.values()), cfg.max_grad_norm)
        self.opt.step()
        self.steps += 1
        if not outputs:
            return None
        det = lambda x: x.detach().clone()   # noqa: E731
        return dict(values=det(t["values"]), log_prob=det(t["log_prob"]), ratio=det(t["ratio"]), grad=grad, grad_norm=float(norm),
                    losses={k: float(t[k].detach()) for k in ("policy_gradient_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "std")})

    def state_dict(self):
        return OrderedDict((k, v.detach().clone()) for k, v in self.p.items())

    def moments(self):
        """(exp_avg, exp_avg_sq) of torch's Adam, dicts by parameter name."""
        st = self.opt.state
        return ({k: st[v]["exp_avg"].clone() for k, v in self.p.items()}, {k: st[v]["exp_avg_sq"].clone() for k, v in self.p.items()})

    def forward(self, obs, cfg, eps=None):
        """(actions, values, log_probs) of ActorCriticPolicy.forward with the sample written as mu + exp(log_std) eps; without eps: deterministic."""
        with torch.no_grad():
            mu, values = heads(self.p, torch.as_tensor(obs).to(self.device, self.dtype), cfg.depth, cfg.separate)
            actions = mu if eps is None else mu + self.p["log_std"].exp() * torch.as_tensor(eps).to(self.device, self.dtype)
            return actions, values, distribution(self.p, mu).log_prob(actions).sum(dim=1)


def adam_from_gradient(params, grad, cfg):
    """clip_grad_norm_ and the first step of torch.optim.Adam(eps=1e-5) in float64 on `params` with the given gradient (dicts by name): (parameters, exp_avg,
    exp_avg_sq, the clip coefficient)."""
    st = RefState(params, torch.float64)
    for g in st.opt.param_groups:
        g["lr"] = cfg.lr
    for k, v in st.p.items():
        v.grad = torch.as_tensor(grad[k]).to(torch.float64).reshape(v.shape).clone()
    norm = float(torch.nn.utils.clip_grad_norm_(list(st.p.values()), cfg.max_grad_norm))
    st.opt.step()
    m, v = st.moments()
    return st.state_dict(), m, v, min(1.0, cfg.max_grad_norm / (norm + 1e-6))


# ---- the cases of the tests
def make_params(obs_dim, act_dim, depth, separate, seed, log_std=-0.5):
    """Parameters under SB3's names with torch.nn.Linear's bounds (uniform in +-1/sqrt(fan_in)), float64 tensors holding float32 values; log_std around `log_std`."""
    g = torch.Generator().manual_seed(int(seed))
    p = OrderedDict()
    lay = layout(obs_dim, act_dim, depth, separate)
    for name, shape in lay.items():
        if name == "log_std":
            p[name] = log_std + 0.2 * (torch.rand(shape, generator=g, dtype=torch.float64) * 2.0 - 1.0)
        else:
            fan_in = lay[name[:name.rindex(".")] + ".weight"][1]
            p[name] = (torch.rand(shape, generator=g, dtype=torch.float64) * 2.0 - 1.0) / math.sqrt(fan_in)
    return OrderedDict((k, v.float().double()) for k, v in p.items())


def make_rows(p, obs, depth, separate, g, clip_range=0.2, clip_range_vf=0.2, margin=0.02):
    """Rows for the observations `obs` [n, K] (float64 holding float32 values): actions drawn from the policy of `p`, and old_log_prob / old_values placed so
    that under `p` the ratio lies inside the clip range (half of the rows, at least `margin` from its ends) or outside (a quarter below, a quarter above, by
    `margin` .. `margin` + 0.13), and the value within clip_range_vf of the old value (half, by `margin`) or beyond.  They are built from the float64 forward
    pass of `p`: inputs, nothing is compared with them.  Returns dict(actions, old_values, old_log_prob, values)."""
    n = obs.shape[0]
    normal = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)   # noqa: E731
    uniform = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)   # noqa: E731
    f32 = lambda x: x.float().double()   # noqa: E731
    with torch.no_grad():
        mu, values = heads(p, obs, depth, separate)
        actions = f32(mu + p["log_std"].exp() * normal(n, mu.shape[1]))
        _, log_prob, _ = evaluate_actions(p, obs, actions, depth, separate)
    kind = torch.randperm(n, generator=g) % 4   # 0, 1: inside; 2: below; 3: above
    c, cv = clip_range, clip_range_vf
    ratio = torch.where(kind < 2, uniform(1.0 - c + margin, 1.0 + c - margin),
                        torch.where(kind == 2, uniform(1.0 - c - margin - 0.13, 1.0 - c - margin), uniform(1.0 + c + margin, 1.0 + c + margin + 0.13)))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    delta = sign * torch.where(torch.randperm(n, generator=g) % 2 == 0, uniform(0.0, cv - margin), uniform(cv + margin, cv + margin + 0.3))
    return dict(actions=actions, old_values=f32(values - delta), old_log_prob=f32(log_prob - torch.log(ratio)), values=values)


def make_case(obs_dim, act_dim, depth, separate, batch, seed, **kw):
    """(params, batch) of one minibatch: observations, make_rows' actions, old values and old log probabilities, advantages of both signs, returns around the values."""
    g = torch.Generator().manual_seed(int(seed) + 1000)
    p = make_params(obs_dim, act_dim, depth, separate, seed)
    f32 = lambda x: x.float().double()   # noqa: E731
    obs = f32(torch.randn(batch, obs_dim, generator=g, dtype=torch.float64))
    rows = make_rows(p, obs, depth, separate, g, **kw)
    values = rows.pop("values")
    b = dict(observations=obs, advantages=f32(torch.randn(batch, generator=g, dtype=torch.float64) + 0.3),
             returns=f32(values + torch.randn(batch, generator=g, dtype=torch.float64)), **rows)
    return p, b


def assert_conditions(out, batch, cfg, tol=1e-3):
    """What the tests ask of their inputs, on a reference's outputs: no row within `tol` of a kink, a quarter of the rows clipped and a quarter not, advantages of
    both signs."""
    ratio, c = out["ratio"].double(), cfg.clip_range
    assert float(torch.minimum((ratio - (1.0 - c)).abs(), (ratio - (1.0 + c)).abs()).min()) >= tol, "a ratio within 1e-3 of the clip range's ends"
    clipped = ((ratio - 1.0).abs() > c).double().mean()
    assert 0.25 <= float(clipped) <= 0.75, f"clipped rows: {float(clipped)}"
    if cfg.clip_range_vf is not None:
        d = (out["values"].double() - torch.as_tensor(batch["old_values"]).double().cpu()).abs()
        assert float((d - cfg.clip_range_vf).abs().min()) >= tol, "a value within 1e-3 of clip_range_vf"
        assert (d > cfg.clip_range_vf).any() and (d < cfg.clip_range_vf).any(), "values on both sides of clip_range_vf"
    adv = torch.as_tensor(batch["advantages"]).double()
    assert (adv > 0).any() and (adv < 0).any(), "advantages of both signs"
