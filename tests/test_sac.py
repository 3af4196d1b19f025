"""The SAC learner, host side: self-checks of tests/sac_ref.py (the torch restatement the device is compared with in tests/test_sac_gpu.py), the config
translation and its refusals, the parameter layout under SB3's names, the descriptor's refusals.  No GPU."""
import math
import os
from types import SimpleNamespace as NS

import pytest
import torch

import sac_ref as R
from human_robot_gym_amd import sac
from human_robot_gym_amd.training_utils import sac_kwargs_from_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference", "training", "config_icra_2024", "environment_evaluation", "training")


def _namespace(node):
    return NS(**{k: _namespace(v) for k, v in node.items()}) if isinstance(node, dict) else node


def _algorithm(**changes):
    import yaml
    alg = yaml.safe_load(open(os.path.join(GOLDEN, "R-SAC.yaml")))["algorithm"]
    alg["seed"] = 3   # (the file interpolates ${run.seed})
    alg.update(changes)
    return NS(algorithm=_namespace(alg))


def test_logp_is_the_normal_log_prob_minus_the_squash_correction():
    g = torch.Generator().manual_seed(0)
    mu, log_std, eps = (torch.randn(50, 4, generator=g, dtype=torch.float64) for _ in range(3))
    a, logp = R.squashed_logp(mu, log_std, eps)
    u = mu + log_std.exp() * eps
    want = torch.distributions.Normal(mu, log_std.exp()).log_prob(u).sum(-1) - torch.log(1.0 - torch.tanh(u) ** 2 + 1e-6).sum(-1)
    torch.testing.assert_close(a, torch.tanh(u), rtol=0, atol=0)
    torch.testing.assert_close(logp, want, rtol=1e-12, atol=1e-12)


def test_adam_update_is_torch_optim_adam_over_three_steps():
    g = torch.Generator().manual_seed(1)
    p0 = torch.randn(7, 5, generator=g, dtype=torch.float64)
    grads = [torch.randn(7, 5, generator=g, dtype=torch.float64) * s for s in (1.0, 1e-3, 10.0)]
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=5e-4)
    for t, gr in enumerate(grads, 1):
        R.adam_update(p, gr, m, v, t, 5e-4)
        q.grad = gr.clone()
        opt.step()
        torch.testing.assert_close(p, q.detach(), rtol=1e-13, atol=1e-15)


def test_the_restatement_moves_targets_on_even_steps_with_interval_two():
    p, batch, e1, e2 = R.make_case(6, 4, 1, 32, seed=2)
    st = R.RefState(p, torch.float64)
    cfg = R.Cfg(1, 5e-4, 0.99, 0.005, True, 0.2, -4.0, 2)
    name = "critic_target.qf0.0.weight"
    moved = []
    for _ in range(4):
        before = st.p[name].clone()
        st.step(batch, e1, e2, cfg)
        moved.append(not torch.equal(before, st.p[name]))
    assert moved == [True, False, True, False]


def test_sac_kwargs_from_the_icra_config():
    kw = sac_kwargs_from_config(_algorithm())
    assert kw == dict(net_arch=[64, 64, 64], learning_rate=0.0005, gamma=0.99, tau=0.005, ent_coef="auto_0.2", target_entropy="auto", batch_size=128,
                      target_update_interval=1, seed=3)
    d = sac.build_sac_desc(6, 4, **{k: v for k, v in kw.items() if k != "learning_rate"})
    assert (d.depth, d.hidden, d.batch_size, d.auto_ent_coef, d.target_update_interval) == (3, 64, 128, 1, 1)
    assert (d.gamma, d.tau, d.ent_coef, d.target_entropy, d.seed) == (0.99, 0.005, 0.2, -4.0, 3)
    assert sac.parse_ent_coef("auto") == (True, 1.0) and sac.parse_ent_coef(0.1) == (False, 0.1)


@pytest.mark.parametrize("changes, key", [
    (dict(use_sde=True), "use_sde"),
    (dict(action_noise=dict(mean=0.0, sigma=0.1)), "action_noise"),
    (dict(policy_kwargs=dict(net_arch=[256, 256])), "net_arch"),
    (dict(policy_kwargs=dict(net_arch=[64, 64, 64, 64])), "net_arch"),
    (dict(policy_kwargs=None), "net_arch"),   # SB3's default [256, 256]
    (dict(policy="CnnPolicy"), "policy"),
])
def test_sac_kwargs_refusals_name_their_key(changes, key):
    with pytest.raises(NotImplementedError, match=key):
        sac_kwargs_from_config(_algorithm(**changes))


@pytest.mark.parametrize("depth", [1, 3])
def test_state_dict_names_and_shapes(depth):
    K, A = 6, 4
    p = sac.SacParams(K, A, depth, seed=5, ent_coef_init=0.2)
    sd = p.state_dict()
    want = {}
    for l in range(depth):
        want[f"actor.latent_pi.{2 * l}.weight"], want[f"actor.latent_pi.{2 * l}.bias"] = (64, 64 if l else K), (64,)
    want.update({"actor.mu.weight": (A, 64), "actor.mu.bias": (A,), "actor.log_std.weight": (A, 64), "actor.log_std.bias": (A,), "log_ent_coef": (1,)})
    for net in ("critic", "critic_target"):
        for q in range(2):
            for l in range(depth):
                want[f"{net}.qf{q}.{2 * l}.weight"], want[f"{net}.qf{q}.{2 * l}.bias"] = (64, 64 if l else K + A), (64,)
            want[f"{net}.qf{q}.{2 * depth}.weight"], want[f"{net}.qf{q}.{2 * depth}.bias"] = (1, 64), (1,)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert sum(v.numel() for k, v in sd.items() if not k.startswith("critic_target.")) == p.n_params == p.params.numel()
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert float(sd["log_ent_coef"]) == pytest.approx(math.log(0.2), rel=1e-7)
    for k, v in sd.items():   # the targets start as copies; the entries are views: writing one writes the flat vector
        if k.startswith("critic."):
            assert torch.equal(v, sd["critic_target." + k[len("critic."):]])
    bound = 1.0 / math.sqrt(K)   # torch.nn.Linear's own initialisation
    w = sd["actor.latent_pi.0.weight"]
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.8 * bound
    sd["actor.mu.bias"].fill_(7.0)
    off = p.layout["actor.mu.bias"][0]
    assert torch.equal(p.params[off:off + A], torch.full((A,), 7.0))
    again = sac.SacParams(K, A, depth, seed=5, ent_coef_init=0.2)   # the same seed: the same weights; another: others; the global generator is left alone
    other = sac.SacParams(K, A, depth, seed=6, ent_coef_init=0.2)
    assert torch.equal(again.state_dict()["critic.qf1.0.weight"], sd["critic.qf1.0.weight"]) and not torch.equal(other.params, again.params)
    torch.manual_seed(9)
    r0 = torch.rand(1)
    torch.manual_seed(9)
    sac.SacParams(K, A, depth, seed=1)
    assert torch.equal(torch.rand(1), r0)
    # round trip through torch modules' own state: load_state_dict(state_dict()) is the identity, a wrong shape or name is refused
    state = {k: v.clone() for k, v in sd.items()}
    other.load_state_dict(state)
    assert torch.equal(other.params, p.params) and torch.equal(other.target, p.target)
    with pytest.raises(KeyError, match="actor.mu.bias"):
        other.load_state_dict({k: v for k, v in state.items() if k != "actor.mu.bias"})
    with pytest.raises(ValueError, match="actor.mu.weight"):
        other.load_state_dict(dict(state, **{"actor.mu.weight": torch.zeros(A, 63)}))


@pytest.mark.parametrize("kwargs, what", [
    (dict(batch_size=48), "batch_size = 48"),
    (dict(batch_size=288), "batch_size = 288"),
    (dict(obs_dim=65), "obs_dim = 65"),
    (dict(net_arch=[64] * 4), "net_arch"),
    (dict(net_arch=[256, 256]), "net_arch"),
    (dict(act_dim=8), "act_dim = 8"),
    (dict(obs_dim=0), "obs_dim = 0"),
])
def test_descriptor_refusals_come_before_any_launch(kwargs, what):
    args = dict(obs_dim=6, act_dim=4, batch_size=128)
    args.update(kwargs)
    with pytest.raises(NotImplementedError, match=what):
        sac.build_sac_desc(**args)
    with pytest.raises(NotImplementedError, match=what):   # the learner builds the descriptor before it touches the device or the library
        sac.SacLearner(**args)


def test_the_header_declares_the_entries_and_only_the_base_unit_includes_the_kernels():
    from human_robot_gym_amd import _lib
    from human_robot_gym_amd._cstruct import PROTOTYPES
    assert {"hrg_sac_create", "hrg_sac_destroy", "hrg_sac_sizes", "hrg_sac_step", "hrg_sac_act", "hrg_sac_export"} <= set(PROTOTYPES)
    for header in ("hrgym_mlp.h", "hrgym_sac.h"):
        including = [os.path.basename(s) for s in _lib.SOURCES if f'#include "{header}"' in open(s).read()]
        assert including == ["hrgym_hip.hip"], header
