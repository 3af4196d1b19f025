"""One behaviour-cloning step (csrc/hrgym_bc.h), restated with torch autograd on the CPU for a SAC actor and for a PPO actor (shared and separate trunk), and the
table of demonstration rows restated in numpy.  Parameterised by dtype, with explicit rows, parameters and Adam state: `ref64` is a float64 run and `ref32` a
float32 run of the same code; their difference is the float32 noise floor the device results are held against (tests/test_bc_gpu.py).  Nothing here reads the
code under test: parameters are a plain dict under SB3's names, the forward passes are sac_ref's and ppo_ref's, Adam is sac_ref.adam_update (torch's Adam,
eps 1e-8), the policy's view of a row is replay_ref.view, the draws come from the tests' counter hash u01 (the oracle's hrgo_test_u01).

    state = RefState(params, "sac" | "ppo", depth, separate, dtype)
    out = state.step(obs, act, lr)       # out["pred"], out["loss"], out["grad"] (dict name -> gradient, zero where the loss does not reach), out["reached"]

The loss is the mean squared error on the deterministic action, averaged over rows and components: SAC mean((tanh(mu(obs)) - a)^2), PPO mean((mu(obs) - a)^2).
Adam moves the entries the loss reaches and nothing else; its moments and step count are this state's own."""
from collections import OrderedDict

import numpy as np
import torch

import ppo_ref
import replay_ref
import sac_ref

STREAM_BC = 15
F32 = np.float32


def prediction(p, obs, kind, depth, separate=False):
    """The deterministic action: SAC tanh(mu), PPO mu."""
    if kind == "sac":
        return torch.tanh(sac_ref.actor_heads(p, obs, depth)[0])
    return ppo_ref.heads(p, obs, depth, separate)[0]


def loss_of(p, obs, act, kind, depth, separate=False):
    return ((prediction(p, obs, kind, depth, separate) - act) ** 2).mean()


class RefState:
    """Parameters, the bc step's own Adam moments and step count of one learner in `dtype`."""

    def __init__(self, params, kind, depth, separate=False, dtype=torch.float64):
        assert kind in ("sac", "ppo")
        self.kind, self.depth, self.separate, self.dtype = kind, int(depth), bool(separate), dtype
        self.p = OrderedDict((k, torch.as_tensor(v).detach().to(dtype).clone()) for k, v in params.items())
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.steps = 0

    def loss(self, obs, act):
        with torch.no_grad():
            return float(loss_of(self.p, torch.as_tensor(obs).to(self.dtype), torch.as_tensor(act).to(self.dtype), self.kind, self.depth, self.separate))

    def step(self, obs, act, lr, outputs=True):
        """One step on the rows `obs` [B, K], `act` [B, A]."""
        p = self.p
        obs, act = torch.as_tensor(obs).detach().to(self.dtype), torch.as_tensor(act).detach().to(self.dtype)
        names = [k for k in p if not k.startswith("critic_target.")]
        for k in names:
            p[k].requires_grad_(True)
        pred = prediction(p, obs, self.kind, self.depth, self.separate)
        loss = ((pred - act) ** 2).mean()
        grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
        for k in names:
            p[k].requires_grad_(False)
        reached = [k for k, g in zip(names, grads) if g is not None]
        grad = {k: torch.zeros_like(v) for k, v in p.items()}
        grad.update({k: g.detach() for k, g in zip(names, grads) if g is not None})
        upd = {}
        with torch.no_grad():
            for k in reached:
                upd[k] = sac_ref.adam_update(p[k], grad[k], self.m[k], self.v[k], self.steps + 1, lr)
        self.steps += 1
        if not outputs:
            return None
        return dict(pred=pred.detach().clone(), loss=float(loss.detach()), grad=grad, reached=reached, update=upd)


# ---- the table of demonstration rows, from the dataset's arrays
def table_rows(ep_offset):
    """(index into the dataset's obs array, t / T_k as float32) of every transition: episode k's observation rows start at ep_offset[k] + k (every episode
    carries one row more than it has transitions: the terminal one, which has no action and is dropped)."""
    rows, time = [], []
    for k in range(len(ep_offset) - 1):
        T = int(ep_offset[k + 1] - ep_offset[k])
        rows += [int(ep_offset[k]) + k + t for t in range(T)]
        time += [F32(t / T) for t in range(T)]
    return np.array(rows, np.int64), np.array(time, F32)


def table(ep_offset, obs, actions, cols, low, high, kind, observe_time=False, mean=None, std=None, squash_factor=None):
    """(observations float32 [total_T, K], actions float32 [total_T, A]) of a dataset's arrays: the policy's view of rows 0 .. T_k - 1 of every episode (the
    columns `cols`, the time value t / T_k behind them with `observe_time`, DatasetObsNormWrapper's arithmetic in double), and the first A = len(low) action
    columns clipped to [low, high]; for SAC brought to [-1, 1] (SB3's scale_action), for PPO left at the env's scale."""
    rows, time = table_rows(ep_offset)
    view = replay_ref.view(np.asarray(obs, F32)[rows], cols, time if observe_time else None, mean, std, squash_factor)
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    a = np.clip(np.asarray(actions, np.float64)[:, :len(low)], low, high)
    if kind == "sac":
        a = 2.0 * ((a - low) / (high - low)) - 1.0
    return view, a.astype(F32)


def draw(u01, seed, step, batch, n_rows):
    """The table rows of bc step number `step` (counted from 0): row k of the batch is floor(u n_rows), clamped to n_rows - 1, u keyed by
    (seed, step, k, STREAM_BC, 0)."""
    return np.array([min(int(np.floor(u01(int(seed), int(step), k, STREAM_BC, 0) * n_rows)), n_rows - 1) for k in range(batch)], np.int64)


# ---- the cases of the tests
def make_params(kind, obs_dim, act_dim, depth, separate, seed):
    """Parameters under SB3's names (sac_ref.make_params / ppo_ref.make_params: float64 tensors holding float32 values).  SAC: two units of the actor's first
    layer are dead on every row (bias -50), so that entries of the gradient are exactly zero."""
    if kind == "sac":
        p = sac_ref.make_params(obs_dim, act_dim, depth, seed)
        p["actor.latent_pi.0.bias"][[3, 17]] = -50.0
        return p
    return ppo_ref.make_params(obs_dim, act_dim, depth, separate, seed)


def make_table(obs_dim, act_dim, n_rows, seed):
    """A table of float32 values: standard normal observations, actions uniform in [-1, 1] with about a fifth of them at exactly -1 or +1 (gripper commands)."""
    g = torch.Generator().manual_seed(int(seed) + 5000)
    obs = torch.randn(n_rows, obs_dim, generator=g, dtype=torch.float64)
    act = torch.rand(n_rows, act_dim, generator=g, dtype=torch.float64) * 2.0 - 1.0
    edge = torch.rand(n_rows, act_dim, generator=g)
    act = torch.where(edge < 0.1, -torch.ones_like(act), torch.where(edge > 0.9, torch.ones_like(act), act))
    return obs.float().numpy(), act.float().numpy()
