"""The host side of the PPO learner (ppo.py, training_utils.ppo_kwargs_from_config) and the anchors of the reference the device is held against (tests/ppo_ref.py).
No GPU: every refusal comes before anything is allocated or launched."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ppo_ref as R
import human_robot_gym_amd as hrg
from human_robot_gym_amd import ppo


# ---- refusals, by message
@pytest.mark.parametrize("kwargs, match", [
    (dict(use_sde=True), "use_sde"),
    (dict(target_kl=0.01), "target_kl"),
    (dict(policy="MultiInputPolicy"), "MlpPolicy"),
    (dict(net_arch=[128, 128]), "widths other than 64"),
    (dict(net_arch=[64, 32]), "widths other than 64"),
    (dict(net_arch=[64] * 4), "depth 4 outside 1 .. 3"),
    (dict(net_arch=[]), "net_arch"),
    (dict(net_arch=[dict(pi=[64], vf=[64, 64])]), "unequal depths"),
    (dict(net_arch=[dict(pi=[64, 64], vf=[64, 128])]), "widths other than 64"),
    (dict(net_arch=[dict(pi=[64] * 4, vf=[64] * 4)]), "depth 4 outside 1 .. 3"),
    (dict(net_arch=[64, dict(pi=[64], vf=[64])]), "mixed arrangement"),
    (dict(net_arch=[dict(pi=[64], vf=[64]), 64]), "last entry"),
    (dict(net_arch=dict(pi=[64], vf=[64])), "net_arch"),
    (dict(net_arch=[dict(pi=[64], vf=[64], qf=[64])]), "unknown keys"),
    (dict(obs_dim=0), "obs_dim = 0"),
    (dict(obs_dim=65), "obs_dim = 65"),
    (dict(act_dim=0), "act_dim = 0"),
    (dict(act_dim=8), "act_dim = 8"),
    (dict(batch_size=16), "batch_size = 16"),
    (dict(batch_size=48), "batch_size = 48"),
    (dict(batch_size=4128), "batch_size = 4128"),
    (dict(batch_size=64, rollout_size=96), "no short last minibatch"),
])
def test_refusals(kwargs, match):
    kw = dict(obs_dim=6, act_dim=7, net_arch=[64, 64])
    kw.update(kwargs)
    with pytest.raises(NotImplementedError, match=match):
        ppo.build_ppo_desc(kw.pop("obs_dim"), kw.pop("act_dim"), **kw)
    kw = dict(obs_dim=6, act_dim=7, net_arch=[64, 64])
    kw.update(kwargs)
    with pytest.raises(NotImplementedError, match=match):   # the learner refuses the same before it opens a device
        ppo.PpoLearner(kw.pop("obs_dim"), kw.pop("act_dim"), **kw)


def test_learner_refuses_unknown_policy_kwargs_and_bad_coefficients():
    with pytest.raises(NotImplementedError, match="sde_net_arch"):
        ppo.PpoLearner(6, 7, net_arch=[64], sde_net_arch=[64])
    with pytest.raises(NotImplementedError, match="activation_fn"):
        ppo.PpoLearner(6, 7, net_arch=[64], activation_fn="relu")
    for bad in (dict(ent_coef=-1.0), dict(vf_coef=float("nan")), dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            ppo.build_ppo_desc(6, 7, net_arch=[64], **bad)
    with pytest.raises(ValueError, match="n_epochs"):
        ppo.PpoLearner(6, 7, net_arch=[64], n_epochs=0)


def test_accepted_descriptors():
    d = ppo.build_ppo_desc(18, 7, net_arch=[64, 64], batch_size=64, rollout_size=4096 * 64, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, seed=3)
    assert (d.obs_dim, d.act_dim, d.depth, d.hidden, d.separate, d.batch_size, d.rollout_size, d.normalize_advantage, d.seed) == (18, 7, 2, 64, 0, 64, 4096 * 64, 1, 3)
    assert (d.use_sde, d.target_kl_set, d.policy) == (0, 0, 0)
    d = ppo.build_ppo_desc(1, 1, batch_size=4096, normalize_advantage=False)   # SB3's default net_arch: separate [64, 64]
    assert (d.depth, d.separate, d.normalize_advantage) == (2, 1, 0)
    for depth in (1, 2, 3):
        assert ppo.parse_net_arch([64] * depth) == (depth, False)
        assert ppo.parse_net_arch([dict(pi=[64] * depth, vf=[64] * depth)]) == (depth, True)


def test_the_header_declares_the_entries_and_only_the_base_unit_includes_the_kernels():
    import os
    from human_robot_gym_amd import _lib
    from human_robot_gym_amd._cstruct import CONST, PROTOTYPES
    assert {"hrg_ppo_create", "hrg_ppo_destroy", "hrg_ppo_sizes", "hrg_ppo_step", "hrg_ppo_forward", "hrg_ppo_export"} <= set(PROTOTYPES)
    assert (CONST["HRG_PPO_HIDDEN"], CONST["HRG_PPO_MAX_DEPTH"], CONST["HRG_PPO_TILE"], CONST["HRG_PPO_MAX_BATCH"], CONST["HRG_PPO_NDIAG"]) == (64, 3, 32, 4096, len(ppo.DIAG_KEYS))
    for header in ("hrgym_mlp.h", "hrgym_ppo.h"):
        including = [os.path.basename(s) for s in _lib.SOURCES if f'#include "{header}"' in open(s).read()]
        assert including == ["hrgym_hip.hip"], header


# ---- layout and names
@pytest.mark.parametrize("separate", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_layout_and_names(depth, separate):
    K, A = 18, 7
    lay, n = ppo.param_layout(K, A, depth, separate)
    nets = ("policy_net", "value_net") if separate else ("shared_net",)
    want = [f"mlp_extractor.{net}.{2 * l}.{x}" for net in nets for l in range(depth) for x in ("weight", "bias")]
    want += ["action_net.weight", "value_net.weight", "action_net.bias", "value_net.bias", "log_std"]
    assert list(lay) == want
    assert n == len(nets) * (64 * K + 64 + (depth - 1) * (64 * 64 + 64)) + (A + 1) * 64 + (A + 1) + A
    off = 0
    for name, (o, shape) in lay.items():   # contiguous, in order
        assert o == off
        off += int(np.prod(shape))
    assert off == n
    assert lay["action_net.weight"][1] == (A, 64) and lay["value_net.weight"][1] == (1, 64) and lay["log_std"][1] == (A,)
    assert lay["value_net.weight"][0] == lay["action_net.weight"][0] + A * 64   # the two heads are one [A + 1][64] product
    assert lay["value_net.bias"][0] == lay["action_net.bias"][0] + A
    # the reference's parameters share the layout
    ref = R.layout(K, A, depth, separate)
    assert list(ref) == list(lay) and all(tuple(ref[k]) == tuple(lay[k][1]) for k in lay)
    assert list(R.make_params(K, A, depth, separate, seed=0)) == list(lay)


@pytest.mark.parametrize("separate", [False, True])
def test_state_dict_views_and_load_identity(separate):
    p = ppo.PpoParams(6, 4, 2, separate, seed=1, log_std_init=-2.7, ortho_init=False)
    sd = p.state_dict()
    assert list(sd) == list(p.layout) and all(tuple(v.shape) == tuple(p.layout[k][1]) for k, v in sd.items())
    assert bool((sd["log_std"] == np.float32(-2.7)).all())
    sd["action_net.bias"][1] = 5.0   # a view: writing into it writes the flat vector
    assert float(p.params[p.layout["action_net.bias"][0] + 1]) == 5.0
    flat = p.params.clone()
    p.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert torch.equal(p.params, flat)
    other = ppo.PpoParams(6, 4, 2, separate, seed=2, ortho_init=False)
    assert not torch.equal(other.params, flat)
    other.load_state_dict({k: v.numpy().copy() for k, v in sd.items()})
    assert torch.equal(other.params, flat)
    with pytest.raises(KeyError, match="missing"):
        p.load_state_dict({k: v for k, v in sd.items() if k != "log_std"})
    with pytest.raises(ValueError, match="shape"):
        p.load_state_dict(dict(sd, log_std=torch.zeros(5)))
    groups = {g: p.group(p.params, g) for g in ppo.GROUPS}
    assert sum(int(v.numel()) for v in groups.values()) == p.n_params
    assert groups["action_net"].numel() == 4 * 64 + 4 and groups["value_net"].numel() == 65 and groups["log_std"].numel() == 4


@pytest.mark.parametrize("separate", [False, True])
def test_both_initialisations(separate):
    K, A, depth = 64, 7, 3
    eye = torch.eye(64, dtype=torch.float64)
    p = ppo.PpoParams(K, A, depth, separate, seed=5, log_std_init=-1.0, ortho_init=True)
    sd = p.state_dict()
    trunk = [k for k in sd if k.startswith("mlp_extractor.") and k.endswith(".weight")]
    assert len(trunk) == depth * (2 if separate else 1)
    for k in trunk:   # orthogonal rows of gain sqrt 2
        W = sd[k].double()
        assert float((W @ W.T - 2.0 * eye).abs().max()) <= 64 * 2.0 ** -22, k
    Wa, Wv = sd["action_net.weight"].double(), sd["value_net.weight"].double()
    assert float((Wa @ Wa.T - 1e-4 * torch.eye(A, dtype=torch.float64)).abs().max()) <= 1e-4 * 64 * 2.0 ** -22
    assert float((Wv @ Wv.T - 1.0).abs().max()) <= 64 * 2.0 ** -22
    assert all(bool((v == 0).all()) for k, v in sd.items() if k.endswith(".bias"))
    assert bool((sd["log_std"] == -1.0).all())
    tall = ppo.PpoParams(6, A, 1, separate, seed=5, ortho_init=True).state_dict()   # [64][6]: orthogonal columns
    for k in tall:
        if k.startswith("mlp_extractor.") and k.endswith(".weight"):
            W = tall[k].double()
            assert float((W.T @ W - 2.0 * torch.eye(6, dtype=torch.float64)).abs().max()) <= 64 * 2.0 ** -22
    # torch.nn.Linear's own: uniform within 1 / sqrt(fan_in), biases not zero; equal seeds equal weights, and the caller's generator is left alone
    torch.manual_seed(123)
    before = torch.rand(1)
    torch.manual_seed(123)
    q = ppo.PpoParams(K, A, depth, separate, seed=5, ortho_init=False)
    assert torch.equal(torch.rand(1), before)
    for k, v in q.state_dict().items():
        if k != "log_std":
            fan_in = q.layout[k[:k.rindex(".")] + ".weight"][1][1]
            assert float(v.abs().max()) <= 1.0 / math.sqrt(fan_in) and float(v.abs().max()) > 0.0, k
    assert torch.equal(q.params, ppo.PpoParams(K, A, depth, separate, seed=5, ortho_init=False).params)
    assert not torch.equal(q.params, ppo.PpoParams(K, A, depth, separate, seed=6, ortho_init=False).params)


# ---- the config reader
def _config(**over):
    """training/config/algorithm/ppo.yaml of the reference, written out."""
    alg = dict(name="PPO", policy="MlpPolicy", learning_rate=7e-5, n_steps=64, batch_size=64, n_epochs=20, gamma=0.99, gae_lambda=0.9, clip_range=0.2, clip_range_vf=None,
               normalize_advantage=True, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, use_sde=False, sde_sample_freq=4, target_kl=None,
               policy_kwargs=dict(net_arch=[64, 64], ortho_init=False, log_std_init=-2.7, full_std=True, use_expln=False, squash_output=True), verbose=1)
    alg.update(over)
    return SimpleNamespace(run=SimpleNamespace(env_type="env"), algorithm=alg)


def test_ppo_kwargs_from_config():
    kw = hrg.ppo_kwargs_from_config(_config())
    assert kw == dict(net_arch=[64, 64], learning_rate=7e-5, batch_size=64, n_epochs=20, clip_range=0.2, clip_range_vf=None, normalize_advantage=True, ent_coef=0.0,
                      vf_coef=0.5, max_grad_norm=0.5, log_std_init=-2.7, ortho_init=False)
    assert hrg.rollout_kwargs_from_config(_config()) == dict(n_steps=64, gamma=0.99, gae_lambda=0.9)
    d = ppo.build_ppo_desc(18, 7, **{k: v for k, v in kw.items() if k in ("net_arch", "batch_size", "normalize_advantage", "ent_coef", "vf_coef", "max_grad_norm")})
    assert (d.depth, d.separate, d.batch_size) == (2, 0, 64)
    # SB3's PPO defaults for what a config leaves out
    kw = hrg.ppo_kwargs_from_config(SimpleNamespace(algorithm=dict(name="PPO")))
    assert kw == dict(net_arch=[dict(pi=[64, 64], vf=[64, 64])], learning_rate=3e-4, batch_size=64, n_epochs=10, clip_range=0.2, clip_range_vf=None,
                      normalize_advantage=True, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, log_std_init=0.0, ortho_init=True)
    assert hrg.ppo_kwargs_from_config(_config(seed=9, clip_range_vf=0.3))["seed"] == 9
    assert hrg.ppo_kwargs_from_config(_config(clip_range_vf=0.3))["clip_range_vf"] == 0.3
    for over, match in ((dict(name="SAC"), "algorithm.name"), (dict(policy="MultiInputPolicy"), "algorithm.policy"), (dict(use_sde=True), "algorithm.use_sde"),
                        (dict(target_kl=0.02), "algorithm.target_kl"), (dict(policy_kwargs=dict(net_arch=[256, 256])), "algorithm.policy_kwargs.net_arch"),
                        (dict(policy_kwargs=dict(net_arch=[64, dict(pi=[64], vf=[64])])), "algorithm.policy_kwargs.net_arch"),
                        (dict(policy_kwargs=dict(net_arch=[64], activation_fn="ReLU")), "activation_fn")):
        with pytest.raises(NotImplementedError, match=match):
            hrg.ppo_kwargs_from_config(_config(**over))


# ---- the reference's own anchors
def test_reference_log_prob_and_entropy_against_the_closed_form():
    K, A, depth = 6, 4, 2
    for separate in (False, True):
        p = R.make_params(K, A, depth, separate, seed=3)
        g = torch.Generator().manual_seed(0)
        obs, act = torch.randn(50, K, generator=g, dtype=torch.float64), torch.randn(50, A, generator=g, dtype=torch.float64)
        values, log_prob, entropy = R.evaluate_actions(p, obs, act, depth, separate)
        mu, v2 = R.heads(p, obs, depth, separate)
        assert torch.equal(values, v2)
        assert float((log_prob - R.log_prob_closed_form(mu, p["log_std"], act)).abs().max()) <= 1e-12
        assert float((entropy - R.entropy_closed_form(p["log_std"])).abs().max()) <= 1e-12
    # one number by hand: a = mu + 2 std in one component with log_std = -1: -2 + 1 - 0.5 log 2 pi
    lp = R.log_prob_closed_form(torch.tensor([[0.3]]), torch.tensor([-1.0]), torch.tensor([[0.3 + 2.0 * math.exp(-1.0)]]))
    assert float(lp) == pytest.approx(-2.0 + 1.0 - 0.5 * math.log(2.0 * math.pi), rel=1e-6)
    n = torch.distributions.Normal(torch.tensor([[0.3]]), torch.tensor([[math.exp(-1.0)]]))
    assert float(n.log_prob(torch.tensor([[0.3 + 2.0 * math.exp(-1.0)]])).sum()) == pytest.approx(float(lp), rel=1e-6)


@pytest.mark.parametrize("separate, normalize, clip_vf", [(False, True, None), (True, False, 0.2)])
def test_reference_gradient_against_finite_differences(separate, normalize, clip_vf):
    K, A, depth, B = 3, 2, 1, 32
    cfg = R.Cfg(depth, separate, 3e-4, 0.2, clip_vf, normalize, 0.01, 0.5, 1e9)
    p, batch = R.make_case(K, A, depth, separate, B, seed=2)
    state = R.RefState(p, torch.float64)
    out = state.step(batch, cfg)
    R.assert_conditions(out, batch, cfg)
    b = R.as_batch(batch, torch.float64)
    value = lambda q: float(R.losses(q, b, cfg)[0])   # noqa: E731
    rng = np.random.RandomState(0)
    h, checked = 1e-6, 0
    for name, g in out["grad"].items():
        flat = g.reshape(-1)
        for i in rng.choice(flat.numel(), size=min(6, flat.numel()), replace=False):
            q = {k: v.clone() for k, v in p.items()}
            q[name].reshape(-1)[i] += h
            up = value(q)
            q[name].reshape(-1)[i] -= 2 * h
            fd = (up - value(q)) / (2 * h)
            assert abs(fd - float(flat[i])) <= 1e-6 * max(1.0, abs(fd)), (name, int(i), fd, float(flat[i]))
            checked += 1
    assert checked >= 25   # six entries of every tensor, all of the shorter ones


def test_reference_clip_coefficient_below_and_above():
    K, A, depth, B = 6, 4, 2, 32
    p, batch = R.make_case(K, A, depth, False, B, seed=4)
    base = R.Cfg(depth, False, 1e-3, 0.2, None, True, 0.01, 0.5, 1e9)
    o = R.RefState(p, torch.float64).step(batch, base)
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in o["grad"].values()))
    assert o["grad_norm"] == pytest.approx(norm, rel=1e-12) and norm > 0
    for max_norm, coef in ((2.0 * norm, 1.0), (0.25 * norm, 0.25 * norm / (norm + 1e-6))):   # below: untouched; above: scaled
        cfg = base._replace(max_grad_norm=max_norm)
        after, m, v, c = R.adam_from_gradient(p, o["grad"], cfg)
        assert c == pytest.approx(coef, rel=1e-12)
        full = R.RefState(p, torch.float64)
        full.step(batch, cfg)
        m2, v2 = full.moments()
        for k in p:   # Adam's first moment after one step is 0.1 x the clipped gradient
            assert float((m[k] - 0.1 * coef * o["grad"][k]).abs().max()) <= 1e-12 * max(1.0, float(o["grad"][k].abs().max()))
            assert torch.allclose(m[k], m2[k], rtol=1e-12, atol=0) and torch.allclose(v[k], v2[k], rtol=1e-12, atol=0)
            assert torch.allclose(after[k], full.state_dict()[k], rtol=1e-12, atol=1e-15)
            upd = (p[k] - after[k]).abs()   # |update| = lr |g| / (|g| + eps sqrt(1 - beta2)...) < lr
            assert float(upd.max()) <= cfg.lr * (1 + 1e-9)
