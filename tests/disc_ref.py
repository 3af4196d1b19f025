"""The discriminator of adversarial imitation (csrc/hrgym_disc.h), restated with torch autograd on the CPU.  Parameterised by dtype, with explicit rows,
parameters and Adam state: `ref64` is a float64 run and `ref32` a float32 run of the same code; their difference is the float32 noise floor the device results
are held against (tests/test_adversarial_gpu.py).  Written from the formulas, not from the kernel, and nothing here reads the code under test: parameters are
a plain dict under the names of a torch Sequential, Adam is sac_ref.adam_update (torch's Adam, eps 1e-8), the draws come from the tests' counter hash u01 (the
oracle's hrgo_test_u01).

    state = RefState(params, depth, activation, dtype)
    out = state.step(expert_obs, expert_act, policy_obs, policy_act, lr)   # out["logits"] [2B] (expert rows first), out["loss"], out["grad"] by name,
                                                                            # out["expert_accuracy"], out["policy_accuracy"]
    r = reward(state.p, obs, act, depth, activation, env_rewards, alpha, kind)

The network: d = head(mlp([obs | act])), `depth` hidden layers of 64 units, ReLU or tanh.  The loss is binary cross-entropy on the logit with the expert's
rows labelled 1: L = (1 / 2B) (sum_expert softplus(-d) + sum_policy softplus(d)).  The reward: softplus(d) = -log(1 - sigmoid(d)) for "gail", d for "airl";
with the env's rewards r_disc alpha + r_env (1 - alpha)."""
from collections import OrderedDict

import numpy as np
import torch

import sac_ref

STREAM_DISC = 17
F32 = np.float32
HIDDEN = 64


def logit(p, obs, act, depth, activation="relu"):
    """d [n]: the logit that a row is the expert's."""
    unit = {"relu": torch.relu, "tanh": torch.tanh}[activation]
    x = torch.cat([obs, act], dim=-1)
    for l in range(depth):
        x = unit(torch.nn.functional.linear(x, p[f"disc.{2 * l}.weight"], p[f"disc.{2 * l}.bias"]))
    return torch.nn.functional.linear(x, p[f"disc.{2 * depth}.weight"], p[f"disc.{2 * depth}.bias"]).squeeze(-1)


def bce(d_expert, d_policy):
    """(1 / 2B) (sum softplus(-d_expert) + sum softplus(d_policy))."""
    sp = torch.nn.functional.softplus
    return (sp(-d_expert).sum() + sp(d_policy).sum()) / (d_expert.numel() + d_policy.numel())


class RefState:
    """Parameters, Adam moments and step count of one discriminator in `dtype`."""

    def __init__(self, params, depth, activation="relu", dtype=torch.float64):
        self.depth, self.activation, self.dtype = int(depth), activation, dtype
        self.p = OrderedDict((k, torch.as_tensor(v).detach().to(dtype).clone()) for k, v in params.items())
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.steps = 0

    def logits(self, obs, act):
        cast = lambda x: torch.as_tensor(x).detach().to(self.dtype)   # noqa: E731
        with torch.no_grad():
            return logit(self.p, cast(obs), cast(act), self.depth, self.activation)

    def step(self, expert_obs, expert_act, policy_obs, policy_act, lr, outputs=True):
        """One update on B expert rows and B policy rows."""
        p = self.p
        cast = lambda x: torch.as_tensor(x).detach().to(self.dtype)   # noqa: E731
        for v in p.values():
            v.requires_grad_(True)
        de = logit(p, cast(expert_obs), cast(expert_act), self.depth, self.activation)
        dp = logit(p, cast(policy_obs), cast(policy_act), self.depth, self.activation)
        loss = bce(de, dp)
        grads = torch.autograd.grad(loss, list(p.values()))
        for v in p.values():
            v.requires_grad_(False)
        grad = {k: g.detach() for k, g in zip(p, grads)}
        upd = {}
        with torch.no_grad():
            for k in p:
                upd[k] = sac_ref.adam_update(p[k], grad[k], self.m[k], self.v[k], self.steps + 1, lr)
        self.steps += 1
        if not outputs:
            return None
        de, dp = de.detach(), dp.detach()
        return dict(logits=torch.cat([de, dp]).clone(), loss=float(loss.detach()), grad=grad, update=upd,
                    expert_accuracy=float((de > 0).double().mean()), policy_accuracy=float((dp < 0).double().mean()))


def reward(p, obs, act, depth, activation="relu", env_rewards=None, alpha=1.0, kind="gail", dtype=torch.float64):
    """(reward [n], logits [n]) of the rows in `dtype`."""
    cast = lambda x: torch.as_tensor(x).detach().to(dtype)   # noqa: E731
    with torch.no_grad():
        d = logit({k: cast(v) for k, v in p.items()}, cast(obs), cast(act), depth, activation)
        r = {"gail": torch.nn.functional.softplus(d), "airl": d}[kind]
        if env_rewards is not None:
            r = r * alpha + cast(env_rewards).reshape(-1) * (1.0 - alpha)
    return r, d


def draw(u01, seed, step, batch, n_rows):
    """The table rows of the expert half of update number `step` (counted from 0): row k is floor(u n_rows), clamped to n_rows - 1, u keyed by
    (seed, step, k, STREAM_DISC, 0)."""
    return np.array([min(int(np.floor(u01(int(seed), int(step), k, STREAM_DISC, 0) * n_rows)), n_rows - 1) for k in range(batch)], np.int64)


# ---- the cases of the tests
def make_params(obs_dim, act_dim, depth, seed):
    """Parameters under the Sequential's names, float64 tensors holding float32 values: a torch.nn.Linear per layer, first to last, under a forked generator
    seeded with `seed` -- the initialisation of the package's learners, so that a state dict moves between the two."""
    p = OrderedDict()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        for l in range(depth + 1):
            lin = torch.nn.Linear(HIDDEN if l else obs_dim + act_dim, HIDDEN if l < depth else 1)
            p[f"disc.{2 * l}.weight"], p[f"disc.{2 * l}.bias"] = lin.weight.detach().double().clone(), lin.bias.detach().double().clone()
    return p


def make_rows(obs_dim, act_dim, n, seed):
    """n rows of float32 values: standard normal observations, actions uniform in [-1, 1]."""
    g = torch.Generator().manual_seed(int(seed) + 7000)
    obs = torch.randn(n, obs_dim, generator=g, dtype=torch.float64)
    act = torch.rand(n, act_dim, generator=g, dtype=torch.float64) * 2.0 - 1.0
    return obs.float().numpy(), act.float().numpy()


SEPARABLE = dict(obs_dim=6, act_dim=4, batch=96, n_rows=37, shift=2.0, seed=5)


def separable_case():
    """(params, table_obs, table_act, indices, policy_obs, policy_act) on which a depth-1 ReLU discriminator separates the halves with a margin: the table's
    rows are Gaussians around +shift in every input, the policy's around -shift; unit j < 32 of the hidden layer reads the mean of the inputs, unit j >= 32
    its negative, the head takes their difference: d = mean(x), so |d| is about `shift` and far above 0.1 on every row (tests/test_adversarial.py checks
    that on ref64).  Every fifth row of the table and every seventh of the policy's lies on the other side, so that neither accuracy is 0 or 1."""
    c = SEPARABLE
    K, A, B, n = c["obs_dim"], c["act_dim"], c["batch"], c["n_rows"]
    g = torch.Generator().manual_seed(c["seed"])
    unit = lambda *shape: (0.3 * torch.randn(*shape, generator=g, dtype=torch.float64)).clamp(-1.0, 1.0)   # noqa: E731
    table, policy = unit(n, K + A) + c["shift"], unit(B, K + A) - c["shift"]
    table[::5] -= 2.0 * c["shift"]
    policy[::7] += 2.0 * c["shift"]
    table, policy = table.float().numpy(), policy.float().numpy()
    p = OrderedDict()
    w = torch.full((HIDDEN, K + A), 1.0 / (K + A), dtype=torch.float64)
    w[HIDDEN // 2:] *= -1.0
    p["disc.0.weight"], p["disc.0.bias"] = w.float().double(), torch.zeros(HIDDEN, dtype=torch.float64)
    head = torch.full((1, HIDDEN), 2.0 / HIDDEN, dtype=torch.float64)
    head[:, HIDDEN // 2:] *= -1.0
    p["disc.2.weight"], p["disc.2.bias"] = head, torch.zeros(1, dtype=torch.float64)
    idx = np.random.RandomState(c["seed"]).randint(0, n, B).astype(np.int64)
    return p, table[:, :K].copy(), table[:, K:].copy(), idx, policy[:, :K].copy(), policy[:, K:].copy()
